"""A seeded batch for dv_pack_draws_device (csrc/pack_regions.hip, pack_draws_kernel) at the level of the C ABI, and
the per-read rule transcribed in plain Python.  Building it needs no GPU.

The batch is what a trimmed, alt-aligned batch of regions looks like to the packer: three "regions" with their own
read names, every candidate owning a row range of its region's TRIMMED table (copies of the reads it overlaps, traced
back to the region's table by src_row), the three trimmed tables concatenated, and behind them an ALT segment whose
rows are copies of trimmed rows (a second src_row hop).  Row keys are integers: a region's key ids (first occurrence
order, as packing.table_key_ids numbers them) shifted by the rows of the regions before it.

  sizes        candidates whose draws have exactly 0, 1, 63, 64, 65, 255, 256 and 257 rows (the wave's edges)
  masks        every candidate is drawn once per mask: draws over the same rows with different masks
  wide         a candidate with 32 alts and a mask with bit 31
  bare         a candidate without support
  both         reads listed under two alts, the larger alt first in list order: first_alt != group
  ghost        support entries whose key no read has
  shared       the SAME read name in region 0 and region 1, supporting alt 0 in one and alt 1 in the other
  alt draws    draws whose rows lie in the alt segment: their keys come through two src_row hops
"""
import numpy as np

from deepvariant_amd import packing

SIZES = (0, 1, 63, 64, 65, 255, 256, 257)
GHOST = 'ghost/0'
SHARED = 'shared/0'
HEIGHT, EXAMPLE_BYTES, SLOT_BYTES = 40, 61 * 40 * 7, 61 * 40 * 7
NO_KEY = -1


class Candidate:
  def __init__(self, region, alts, masks):
    self.region = region
    self.alts = list(alts)                # allele strings
    self.masks = [int(m) for m in masks]
    self.support = []                     # (key string, alt index), in list order
    self.rows = (0, 0)                    # its range of the concatenated table (trimmed)
    self.alt_rows = {}                    # alt index -> its range of the concatenated table (alt segment)


class Batch:
  """Everything the call takes, and what it was made from."""


def _masks(n_alts):
  singles = [1 << i for i in range(n_alts)]
  return (singles + [(1 << i) | (1 << j) for i in range(n_alts) for j in range(i + 1, n_alts)])[:6]


def _first_occurrence_ids(keys):
  ids = {}
  return np.array([ids.setdefault(k, len(ids)) for k in keys], np.int32).reshape(len(keys)), ids


def build(seed=11, shift_rows=True):
  """`shift_rows=False` leaves the ROW keys of every region unshifted while the support keys stay shifted: the key
  leak the shared read is there to catch."""
  rng = np.random.default_rng(seed)
  b = Batch()
  # ---- the regions' own tables: names, some keys shared by two rows, the shared name in regions 0 and 1
  b.region_keys = []
  for k, n in enumerate((300, 420, 330)):
    names = ['r%d_%d/%d' % (k, i, i % 2) for i in range(n - 20)]
    names += [names[int(i)] for i in rng.integers(0, n - 20, size=20)]      # two rows, one key
    order = rng.permutation(n)
    keys = [names[int(i)] for i in order]
    if k < 2:
      keys[17 + k] = SHARED
    b.region_keys.append(keys)
  key_base = np.concatenate([[0], np.cumsum([len(k) for k in b.region_keys])])[:-1].astype(np.int64)
  # ---- candidates: one per size, spread over the regions; then wide and bare
  cands = []
  for j, size in enumerate(SIZES):
    n_alts = 1 + j % 3
    cands.append((Candidate(j % 3, ['A' * (i + 2) for i in range(n_alts)], _masks(n_alts)), size))
  wide = Candidate(1, ['C' * (i + 1) for i in range(32)], [1 << 31, (1 << 31) | 1, 1])
  cands.append((wide, 70))
  bare = Candidate(2, ['G', 'GT'], _masks(2))
  cands.append((bare, 40))
  shared_cands = [Candidate(0, ['T', 'TT'], _masks(2)), Candidate(1, ['T', 'TT'], _masks(2))]
  cands += [(c, 30) for c in shared_cands]
  cands.sort(key=lambda cs: cs[0].region)                                    # region order, as the route lists them
  b.cands = [c for c, _ in cands]
  # ---- trimmed rows: per candidate a range of copies of its region's rows, ascending by source row
  b.trimmed_src = [[] for _ in b.region_keys]      # per region: source row of every trimmed row
  per_region_rows = [0, 0, 0]
  for cand, size in cands:
    n = len(b.region_keys[cand.region])
    src = np.sort(rng.choice(n, size=size, replace=False))
    if cand in shared_cands and 17 + cand.region not in src.tolist():
      src[0] = 17 + cand.region
      src = np.sort(src)
    cand.local = (per_region_rows[cand.region], size)
    cand.src = src
    b.trimmed_src[cand.region].append(src)
    per_region_rows[cand.region] += size
  b.trimmed_src = [np.concatenate(p).astype(np.int32) if p else np.zeros(0, np.int32) for p in b.trimmed_src]
  row_base = np.concatenate([[0], np.cumsum(per_region_rows)])[:-1]
  b.n_trimmed = int(sum(per_region_rows))
  for cand, _ in cands:
    cand.rows = (int(row_base[cand.region]) + cand.local[0], cand.local[1])
  # ---- support, by key string
  for cand, size in cands:
    keys = b.region_keys[cand.region]
    n_alts = len(cand.alts)
    if cand is bare:
      continue
    support = []
    for r in cand.src.tolist():
      draw = int(rng.integers(0, 4))
      if draw == 0:
        continue                                                      # supports the reference
      support.append((keys[r], int(rng.integers(0, n_alts))))
    if n_alts >= 2 and size >= 2:
      for r in cand.src[:max(2, size // 8)].tolist():                  # listed under two alts, the larger FIRST
        support = [(k, a) for k, a in support if k != keys[r]]
        support += [(keys[r], n_alts - 1), (keys[r], 0)]
    if cand is wide:
      support = [(keys[r], 31 if i % 2 else 0) for i, r in enumerate(cand.src.tolist())]
      support += [(keys[int(cand.src[7])], 0), (keys[int(cand.src[8])], 31)]
    if cand in shared_cands:
      support = [(k, a) for k, a in support if k != SHARED] + [(SHARED, cand.region)]      # alt 0 here, alt 1 there
    support += [(GHOST, a) for a in range(min(n_alts, 2))]
    support += [(keys[int(r)], 0) for r in rng.integers(0, len(keys), size=3)]               # reads it does not draw
    cand.support = [support[int(i)] for i in rng.permutation(len(support))]
    if n_alts >= 2 and size >= 2 and cand is not wide:
      # list order decides nothing: put one pair back larger-alt-first explicitly
      k0 = next(keys[int(r)] for r in cand.src.tolist() if keys[int(r)] != SHARED)
      cand.support = [(k, a) for k, a in cand.support if k != k0] + [(k0, n_alts - 1), (k0, 0)]
  # ---- the alt segment: per (candidate, alt) of a few candidates, copies of most of its trimmed rows
  alt_src = []
  n_alt = 0
  for cand, size in cands:
    if size not in (64, 65, 256, 257) and cand not in shared_cands:
      continue
    for ai in range(min(len(cand.alts), 2)):
      first, n = cand.rows
      keep = np.sort(rng.choice(n, size=n - n // 10, replace=False)) + first          # the aligner drops some
      cand.alt_rows[ai] = (b.n_trimmed + n_alt, len(keep))
      alt_src.append(keep)
      n_alt += len(keep)
  b.alt_src = np.concatenate(alt_src).astype(np.int32)                # rows of the concatenated trimmed table
  b.n_rows = b.n_trimmed + n_alt
  # ---- integer keys: a region's first-occurrence ids, shifted; two hops for the alt segment
  region_ids, b.id_of = [], []
  for keys in b.region_keys:
    ids, table = _first_occurrence_ids(keys)
    region_ids.append(ids)
    b.id_of.append(table)
  trimmed_key = np.concatenate([region_ids[k][b.trimmed_src[k]].astype(np.int64) + (key_base[k] if shift_rows else 0)
                                for k in range(3)])
  b.rows_key = np.ascontiguousarray(np.concatenate([trimmed_key, trimmed_key[b.alt_src]]), np.int32)
  b.key_base = key_base
  b.n_alts = np.array([len(c.alts) for c in b.cands], np.int32)
  first, count, skey, salt = [], [], [], []
  for c in b.cands:
    first.append(len(skey))
    count.append(len(c.support))
    for key, alt in c.support:
      local = b.id_of[c.region].get(key, NO_KEY)
      skey.append(NO_KEY if local == NO_KEY else local + int(key_base[c.region]))
      salt.append(alt)
  b.first_support, b.n_support = np.array(first, np.uint32), np.array(count, np.uint32)
  b.support_key, b.support_alt = np.array(skey, np.int32), np.array(salt, np.uint8)
  # ---- draws: the reference images first (one per candidate and mask), the alt images behind them
  ref, alt = [], []
  b.kinds = []
  for ci, c in enumerate(b.cands):
    for mask in c.masks:
      ref.append((ci, mask, c.rows[0], c.rows[1], ci, 1000 * ci, 1000 * ci - 30, HEIGHT, len(ref) * EXAMPLE_BYTES,
                  0.5 * ci))
      for ai in [i for i in range(len(c.alts)) if (mask >> i) & 1][:2]:
        if ai in c.alt_rows:
          alt.append((ci, mask, c.alt_rows[ai][0], c.alt_rows[ai][1], len(b.cands) + len(alt), 1000 * ci,
                      1000 * ci - 30, HEIGHT, len(alt) * SLOT_BYTES, 0.5 * ci))
  b.n_examples = len(ref)
  b.draws = np.array(ref + alt, packing.DRAW_DTYPE)
  b.draws['out_off'][b.n_examples:] += np.uint64(b.n_examples * EXAMPLE_BYTES)
  return b


_BATCH = None


def batch():
  """The batch every test shares (never modified)."""
  global _BATCH
  if _BATCH is None:
    _BATCH = build()
  return _BATCH


def key_string(b, row):
  """The key string of a row of the concatenated table, and its region: through src_row, twice for an alt row."""
  if row >= b.n_trimmed:
    row = int(b.alt_src[row - b.n_trimmed])
  at = 0
  for k, src in enumerate(b.trimmed_src):
    if row < at + len(src):
      return b.region_keys[k][int(src[row - at])], k
    at += len(src)
  raise IndexError(row)


def transcription(rows_key, draws, n_alts, first_support, n_support, support_key, support_alt):
  """The per-read rule of include/dvhip.h, read off the integer arrays the device gets -> the handle's arrays by
  dv_batch field name (+ item_candidate, item_combo, max_list_len)."""
  n = len(draws)
  out = dict(item_variant_start=draws['variant_start'].astype(np.int32), item_image_start=draws['image_start'].astype(np.int32),
             item_ref_idx=draws['ref_idx'].astype(np.uint32), item_height=draws['height'].astype(np.uint16),
             item_out_off=draws['out_off'].astype(np.uint64), item_mean_coverage=draws['mean_coverage'].astype(np.float32),
             item_candidate=draws['cand'].astype(np.int32), item_combo=draws['combo_mask'].astype(np.uint32))
  off = np.zeros(n + 1, np.int64)
  np.cumsum(draws['n_rows'].astype(np.int64), out=off[1:])
  out['item_list_off'] = off.astype(np.uint32)
  reads, codes, groups = [], [], []
  for d in draws:
    c = int(d['cand'])
    lo, cnt = int(first_support[c]), int(n_support[c])
    entries = list(zip(support_key[lo:lo + cnt].tolist(), support_alt[lo:lo + cnt].tolist()))
    mask = int(d['combo_mask'])
    for row in range(int(d['row_first']), int(d['row_first']) + int(d['n_rows'])):
      key = int(rows_key[row]) if rows_key is not None else row
      mine = [alt for k, alt in entries if k == key]
      first_alt, group = (min(mine), max(mine)) if mine else (255, int(n_alts[c]))
      reads.append(row)
      codes.append(0 if first_alt == 255 else 1 if (mask >> first_alt) & 1 else 2)
      groups.append(group)
  out['list_read'] = np.array(reads, np.uint32)
  out['list_code'] = np.array(codes, np.uint8)
  out['list_group'] = np.array(groups, np.uint8)
  out['max_list_len'] = int(draws['n_rows'].max()) if n else 0
  return out


_WANT = None


def expected():
  """transcription() of the shared batch, computed once."""
  global _WANT
  if _WANT is None:
    b = batch()
    _WANT = transcription(b.rows_key, b.draws, b.n_alts, b.first_support, b.n_support, b.support_key, b.support_alt)
  return _WANT


def call(b, stream=None, rows_key='given', **override):
  """dv_pack_draws_device on the batch's arrays (fields replaced by `override`) -> packing.PackedRegions."""
  args = dict(draws=b.draws, n_alts=b.n_alts, first_support=b.first_support, n_support=b.n_support,
              support_key=b.support_key, support_alt=b.support_alt, n_rows=b.n_rows)
  args.update(override)
  return packing.pack_draws_device(b.rows_key if isinstance(rows_key, str) else rows_key, args['n_rows'], args['draws'],
                                   args['n_alts'], args['first_support'], args['n_support'], args['support_key'],
                                   args['support_alt'], stream=stream)
