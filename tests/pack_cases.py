"""Seeded regions for the device packer (dv_pack_regions_device, csrc/pack_regions.hip) at the level of the C ABI,
the host checker's answer for them (dv_pack_region, keys rendered as strings) and the batch-wide arrays the
device must return.  Building a case needs no GPU.

  generator_region   the generator of tests/test_region_packer_cpu.py: 700 reads under 300 fragment names (keys are
                     shared), 60 candidates including duplicates and candidates without a reference window, 1-3
                     alts, reads listed under several alts, a ghost key; rows shuffled or sorted, and in the sorted
                     form one read long enough to reach every candidate from far in front of it
  pile_region        1,100 reads on one position
  edges_region       candidates whose lists have exactly 0, 1, 63, 64, 65, 255, 256, 257, 1,024 and 1,025 reads
                     (the wave and chunk edges), and a candidate with 32 alts and a mask with bit 31 set
  empty_region / no_candidates_region
"""
import ctypes as C

import numpy as np

from deepvariant_amd import _lib

WIDTH, BUFFER, HEIGHT, EXAMPLE_BYTES = 61, 5, 40, 61 * 40 * 7
EDGE_SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 1024, 1025)
GHOST = 'ghost/0'


class Candidate:
  def __init__(self, start, end, n_alts, masks, support, window=True):
    self.start, self.end, self.n_alts = int(start), int(end), int(n_alts)
    self.masks = [int(m) for m in masks]
    self.support = [(str(k), int(a)) for k, a in support]     # (key string, alt index), in list order
    self.window = bool(window)


class Region:
  def __init__(self, name, read_pos, read_end, names, read_number, candidates):
    self.name = name
    self.read_pos = np.ascontiguousarray(read_pos, np.int32)
    self.read_end = np.ascontiguousarray(read_end, np.int64)
    self.names = list(names)
    self.read_number = np.ascontiguousarray(read_number, np.uint8)
    self.candidates = list(candidates)

  @property
  def n_reads(self):
    return len(self.names)

  @property
  def keys(self):
    return ['%s/%d' % (n, r) for n, r in zip(self.names, self.read_number.tolist())]

  @property
  def sorted(self):
    return bool(np.all(np.diff(self.read_pos.astype(np.int64)) >= 0))

  def picked(self, cand):
    """Rows the candidate's query picks, ascending (the contract's predicate, in numpy)."""
    return np.nonzero((cand.end + BUFFER > self.read_pos.astype(np.int64)) & (cand.start - BUFFER < self.read_end))[0]

  def key_ids(self):
    """int32 per row from the key strings, and the dict behind it."""
    ids = {}
    per_row = np.array([ids.setdefault(k, len(ids)) for k in self.keys], np.int32).reshape(self.n_reads)
    return per_row, ids


def _all_masks(n_alts, rng=None):
  """One mask per alt and per pair of alts (ADD_HET_ALT_IMAGES' combinations), capped for wide sites."""
  masks = [1 << i for i in range(n_alts)] + [(1 << i) | (1 << j) for i in range(n_alts) for j in range(i + 1, n_alts)]
  return masks[:6]


def generator_region(seed, shuffle):
  rng = np.random.default_rng(seed)
  n = 700
  pos = rng.integers(0, 2900, size=n)
  span = rng.integers(1, 400, size=n)
  names = ['f%d' % int(x) for x in rng.integers(0, 300, size=n)]
  number = rng.integers(0, 2, size=n)
  if not shuffle:
    order = np.argsort(pos, kind='stable')
    pos, span, number = pos[order], span[order], number[order]
    names = [names[i] for i in order]
    # a read that starts far in front of the candidates it reaches: the sorted bound needs the largest span
    pos[0], span[0] = 0, 2950
  region = Region('generator-%s' % ('shuffled' if shuffle else 'sorted'), pos, pos + span, names, number, [])
  keys = region.keys
  positions = rng.integers(0, 2990, size=56).tolist()
  for k, p in enumerate(sorted(positions + positions[:4])):                     # duplicates included
    n_alts = int(rng.integers(1, 4))
    cand = Candidate(p, p + 1, n_alts, _all_masks(n_alts), [], window=not (p < 30 or p > 2960 or k % 17 == 5))
    near = region.picked(cand)
    support = []
    for alt in range(n_alts):
      # mostly reads the candidate picks, some it does not, a ghost
      rows = list(rng.choice(near, size=min(len(near), int(rng.integers(0, 25))), replace=False)) if len(near) else []
      rows += rng.integers(0, n, size=int(rng.integers(0, 6))).tolist()
      support += [(keys[int(r)], alt) for r in rows] + [(GHOST, alt)]
    if n_alts >= 2 and len(near):
      # reads listed under several alts, the larger alt FIRST in list order: first_alt is the smallest, group the largest
      for r in rng.choice(near, size=min(len(near), 8), replace=False):
        support += [(keys[int(r)], n_alts - 1), (keys[int(r)], 0)]
    order = rng.permutation(len(support))
    cand.support = [support[int(i)] for i in order]
    region.candidates.append(cand)
  return region


def pile_region(seed=3):
  rng = np.random.default_rng(seed)
  n = 1100
  pos = np.full(n, 5000)
  names = ['p%d' % i for i in range(n)]
  region = Region('pile', pos, pos + rng.integers(50, 151, size=n), names, np.zeros(n, np.uint8), [])
  keys = region.keys
  for p, n_alts in ((4990, 1), (5020, 2), (5100, 3), (5160, 1)):
    support = [(keys[int(r)], int(rng.integers(0, n_alts))) for r in rng.integers(0, n, size=300)]
    region.candidates.append(Candidate(p, p + 2, n_alts, _all_masks(n_alts), support))
  return region


def edges_region():
  pos, names, cands = [], [], []
  for k, size in enumerate(EDGE_SIZES):
    at = 10000 * (k + 1)
    pos += [at] * size
    names += ['e%d_%d' % (size, i) for i in range(size)]
    # every second read supports alt 0, every third alt 1 (so every sixth is listed under both)
    support = [('e%d_%d/0' % (size, i), 0) for i in range(0, size, 2)] + [('e%d_%d/0' % (size, i), 1) for i in range(0, size, 3)]
    cands.append(Candidate(at + 50, at + 51, 2, [1, 2, 3], support))
  # 32 alts, a mask with bit 31: on the 65-read pile
  at = 10000 * (EDGE_SIZES.index(65) + 1)
  support = [('e65_%d/0' % i, 31 if i % 2 else 0) for i in range(65)] + [('e65_7/0', 0), ('e65_8/0', 31)]
  cands.append(Candidate(at + 60, at + 61, 32, [1 << 31, (1 << 31) | 1, 1], support))
  cands.sort(key=lambda c: c.start)
  pos = np.array(pos, np.int64)
  return Region('edges', pos, pos + 100, names, np.zeros(len(names), np.uint8), cands)


def empty_region():
  """No reads; its candidate gives items with empty lists."""
  return Region('empty', [], [], [], [], [Candidate(100, 101, 1, [1], [(GHOST, 0)])])


def no_candidates_region(seed=9):
  rng = np.random.default_rng(seed)
  pos = np.sort(rng.integers(0, 1000, size=50))
  return Region('no-candidates', pos, pos + 100, ['n%d' % i for i in range(50)], np.zeros(50, np.uint8), [])


_BATCH = None


def batch():
  """The batch every test shares: full regions with an empty one and one without candidates between them."""
  global _BATCH
  if _BATCH is None:
    _BATCH = [generator_region(5, shuffle=False), empty_region(), generator_region(6, shuffle=True),
              no_candidates_region(), pile_region(), edges_region()]
  return _BATCH


# ---- the checker: dv_pack_region on one region, keys as strings
_ARRAYS = (('item_variant_start', np.int32), ('item_image_start', np.int32), ('item_ref_idx', np.uint32),
           ('item_list_off', np.uint32), ('item_height', np.uint16), ('item_out_off', np.uint64))


def _copy(ptr, dtype, count):
  if not count:
    return np.zeros(0, dtype)
  return np.frombuffer((C.c_char * (count * np.dtype(dtype).itemsize)).from_address(ptr), dtype, count).copy()


def host_pack(region, use_groups, threads=1):
  """dv_pack_region's arrays for one region -> dict by dv_batch field name (+ item_candidate, item_combo,
  max_list_len, n_windows)."""
  lib = _lib.lib()
  raw = [n.encode() for n in region.names]
  blob = np.frombuffer(b'\0'.join(raw) + b'\0', np.uint8).copy()
  offs = np.concatenate([[0], np.cumsum([len(x) + 1 for x in raw])[:-1]]).astype(np.uint32) if raw else np.zeros(1, np.uint32)
  reads = _lib.DvPackReads(region.n_reads, region.read_pos.ctypes.data, region.read_end.ctypes.data, blob.ctypes.data,
                           offs.ctypes.data, region.read_number.ctypes.data)
  opt = _lib.DvPackOptions(WIDTH, BUFFER, HEIGHT, threads, EXAMPLE_BYTES)
  n = len(region.candidates)
  cands = (_lib.DvPackCandidate * max(n, 1))()
  masks, keys, alts, n_windows = [], [], [], 0
  for i, cand in enumerate(region.candidates):
    c = cands[i]
    c.start, c.end, c.n_alts = cand.start, cand.end, cand.n_alts
    c.ref_idx = -1
    if cand.window:
      c.ref_idx = n_windows
      n_windows += 1
    c.first_combo, c.n_combos = len(masks), len(cand.masks)
    masks += cand.masks
    c.first_support, c.n_support = len(keys), len(cand.support)
    keys += [k.encode() for k, _ in cand.support]
    alts += [a for _, a in cand.support]
  mask_arr = np.array(masks or [0], np.uint32)
  key_blob = np.frombuffer(b'\0'.join(keys) + b'\0', np.uint8).copy()
  key_off = np.concatenate([[0], np.cumsum([len(k) + 1 for k in keys])[:-1]]).astype(np.uint32) if keys else np.zeros(1, np.uint32)
  alt_arr = np.array(alts or [0], np.uint8)
  handle = C.c_void_p()
  _lib.check(lib.dv_pack_region(C.byref(reads), C.byref(opt), n, cands, mask_arr.ctypes.data, key_blob.ctypes.data,
                                key_off.ctypes.data, alt_arr.ctypes.data, C.byref(handle)))
  try:
    b = _lib.DvBatch()
    _lib.check(lib.dv_packed_region_fill_batch(handle, int(use_groups), C.byref(b)))
    ic, im = C.c_void_p(), C.c_void_p()
    n_items = lib.dv_packed_region_items(handle, C.byref(ic), C.byref(im))
    out = {name: _copy(getattr(b, name), dtype, n_items + (name == 'item_list_off')) for name, dtype in _ARRAYS}
    if not n_items:
      out['item_list_off'] = np.zeros(1, np.uint32)
    out['list_read'] = _copy(b.list_read, np.uint32, b.n_list)
    out['list_code'] = _copy(b.list_code, np.uint8, b.n_list)
    out['list_group'] = _copy(b.list_group, np.uint8, b.n_list) if use_groups else None
    out['item_candidate'] = _copy(ic.value, np.int32, n_items)
    out['item_combo'] = _copy(im.value, np.uint32, n_items)
    out['max_list_len'] = int(b.max_list_len)
    out['n_windows'] = n_windows
    return out
  finally:
    lib.dv_packed_region_free(handle)


def expected(regions, use_groups):
  """What the device returns for the batch: the regions' host arrays one after the other, rows shifted by the
  region's first row, list offsets by the entries before, reference windows and candidates by those before, and
  item_out_off by item number."""
  parts = [host_pack(r, use_groups) for r in regions]
  out = {}
  rows = lists = windows = cands = 0
  acc = {name: [] for name in ('item_variant_start', 'item_image_start', 'item_ref_idx', 'item_height', 'item_candidate',
                               'item_combo', 'list_read', 'list_code', 'list_group')}
  offs = [np.zeros(1, np.uint32)]
  for region, p in zip(regions, parts):
    for name in acc:
      if p[name] is not None:
        acc[name].append(p[name])
    acc['item_ref_idx'][-1] = (p['item_ref_idx'] + windows).astype(np.uint32)
    acc['item_candidate'][-1] = (p['item_candidate'] + cands).astype(np.int32)
    acc['list_read'][-1] = (p['list_read'] + rows).astype(np.uint32)
    offs.append((p['item_list_off'][1:].astype(np.int64) + lists).astype(np.uint32))
    rows += region.n_reads
    lists += len(p['list_read'])
    windows += p['n_windows']
    cands += len(region.candidates)
  for name, chunks in acc.items():
    out[name] = np.concatenate(chunks) if chunks else None
  out['item_list_off'] = np.concatenate(offs)
  n_items = len(out['item_height'])
  out['item_out_off'] = (np.arange(n_items, dtype=np.uint64) * np.uint64(EXAMPLE_BYTES)).astype(np.uint64)
  out['max_list_len'] = max([p['max_list_len'] for p in parts] or [0])
  return out


# ---- the device call's inputs
class DeviceInputs:
  """The arrays dv_pack_regions_device takes for `regions` (kept alive here)."""

  def __init__(self, regions, mean_coverage=0.0, with_keys=True):
    n_reads = sum(r.n_reads for r in regions)
    cat = lambda parts, dtype: (np.ascontiguousarray(np.concatenate(parts), dtype) if parts else np.zeros(0, dtype))    # noqa: E731
    self.read_pos = cat([r.read_pos for r in regions], np.int32)
    self.read_end = cat([r.read_end for r in regions], np.int64)
    n_cands = sum(len(r.candidates) for r in regions)
    self.slices = (_lib.DvPackRegionSlice * max(len(regions), 1))()
    self.cands = (_lib.DvPackCandidate * max(n_cands, 1))()
    key_parts, masks, skeys, salts = [], [], [], []
    row0 = ci = windows = 0
    for k, region in enumerate(regions):
      per_row, ids = region.key_ids()
      if not with_keys:
        # NULL read_key: a row is its own key, named by its row in the concatenated table (only for regions
        # whose keys all differ)
        assert len(ids) == region.n_reads
        ids = {key: row0 + row for key, row in ids.items()}
      key_parts.append(per_row)
      s = self.slices[k]
      s.read_first, s.n_reads, s.cand_first, s.n_cands = row0, region.n_reads, ci, len(region.candidates)
      for cand in region.candidates:
        c = self.cands[ci]
        c.start, c.end, c.n_alts = cand.start, cand.end, cand.n_alts
        c.ref_idx = -1
        if cand.window:
          c.ref_idx = windows
          windows += 1
        c.first_combo, c.n_combos = len(masks), len(cand.masks)
        masks += cand.masks
        c.first_support, c.n_support = len(skeys), len(cand.support)
        skeys += [ids.get(key, -1) for key, _ in cand.support]       # a ghost matches no row
        salts += [alt for _, alt in cand.support]
        ci += 1
      row0 += region.n_reads
    self.read_key = cat(key_parts, np.int32) if with_keys else None
    self.masks = np.array(masks or [0], np.uint32)
    self.support_key = np.array(skeys or [0], np.int32)
    self.support_alt = np.array(salts or [0], np.uint8)
    self.rows = _lib.DvPackRows(n_reads, self.read_pos.ctypes.data, self.read_end.ctypes.data,
                                self.read_key.ctypes.data if self.read_key is not None else None)
    self.opt = _lib.DvPackRegionsOptions(WIDTH, BUFFER, HEIGHT, n_cands, len(masks), len(skeys), EXAMPLE_BYTES,
                                         float(mean_coverage))
    self.n_regions = len(regions)

  def call(self, stream=None):
    """-> (status, handle)."""
    handle = C.c_void_p()
    status = _lib.lib().dv_pack_regions_device(
        self.n_regions, self.slices, C.byref(self.rows), C.byref(self.opt), self.cands, self.masks.ctypes.data,
        self.support_key.ctypes.data, self.support_alt.ctypes.data, C.c_void_p(stream) if stream else None,
        C.byref(handle))
    return status, handle
