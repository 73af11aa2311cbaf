"""The proof, from the host's answers alone, that the cases of tests/batch_edge_cases.py hold what
tests/test_hip_batch_edges.py depends on: exactly the advertised number of elements, something to carry across the
step of every scan (pairs with words, kept pairs, candidates with items and lists on both sides of element 1,024),
the element whose own count is 0 on the edge, a window whose first pair is pair 1,024, the longest list behind the
second carry -- and that the host checkers used there are pinned once to an independent restatement.  No GPU."""
import numpy as np
import pytest

from deepvariant_amd import alt_aligned_pileup_lib as A
from tests import alt_align_cases as AC
from tests import batch_edge_cases as E
from tests import pack_cases as PC
from tests import trim_cases as TC

STEP = E.SCAN_STEP
_ALT_HOST = {}


def _alt_host(n_pairs, normalize_reads=0):
  key = (n_pairs, normalize_reads)
  if key not in _ALT_HOST:
    b = E.edge_alt_align(n_pairs)
    _ALT_HOST[key] = A.alt_align_arrays(E.alt_align_table(n_pairs), b['items'], b['targets'],
                                        dict(b['cfg'], normalize_reads=normalize_reads), device=False)
  return _ALT_HOST[key]


# ---------------------------------------------------------------- alt-align
@pytest.mark.parametrize('n_pairs', E.SCAN_SIZES)
def test_alt_align_cases_hold_the_pairs_they_promise(n_pairs):
  b = E.edge_alt_align(n_pairs)
  d = _alt_host(n_pairs)
  assert int(d['item_pair_off'][-1]) == n_pairs == len(d['status']) == sum(it[1] for it in b['items'])
  assert len(b['reads']) == 100 and all(8 <= len(r.aligned_sequence) <= 60 for r in b['reads'][:96])
  assert all(70 <= len(t) <= 90 for t in b['targets'][:5])
  words = np.diff(d['cigar_off'].astype(np.int64))
  status = d['status']
  assert 0 <= words.min() and words.max() >= 20 and (words[status != 1] == 0).all()
  assert set(status[:STEP].tolist()) == {0, 1, 2}
  assert d['cigar_off'][min(STEP, n_pairs)] > 0                      # what the first step hands to the second
  for edge in (STEP, 2 * STEP):
    if n_pairs > edge:
      # the last pair of one step and the first of the next both write words, behind a carry that is not 0
      assert words[edge - 1] > 0 and words[edge] > 0 and d['cigar_off'][edge] > d['cigar_off'][edge - STEP]
  if n_pairs >= 2 * STEP:
    # every status on both sides of the first edge (the 1,025-pair case has one pair behind it: status 1)
    assert set(status[STEP:].tolist()) == {0, 1, 2}
  # with normalize_reads the pair of kind `unnormalised` moves (status 1): the words before the edge differ
  assert _alt_host(n_pairs, 1)['cigar_off'][min(STEP, n_pairs)] > d['cigar_off'][min(STEP, n_pairs)]


def test_alt_align_host_entry_equals_the_object_route_on_1025_pairs():
  """The checker of the GPU tests, pinned once to fast_pass_aligner.realign_reads_to_haplotype on Read objects."""
  from tests.test_alt_align_abi_cpu import _pairs
  b = E.edge_alt_align(1025)
  for normalize_reads in (0, 1):
    d = _alt_host(1025, normalize_reads)
    want = AC.object_route(b, bool(normalize_reads))
    for item, (first, n_rows, _, _, _) in enumerate(b['items']):
      got = _pairs(d, item)
      assert len(got) == n_rows == len(want[item])
      for row, ((status, position, cigar), read) in enumerate(zip(got, want[item])):
        if read is None:
          assert (status, position, cigar) == (2, 0, []), (item, row)
        elif read is b['reads'][first + row]:
          assert (status, position, cigar) == (0, 0, []), (item, row)
        else:
          assert status == 1 and position == read.alignment.position.position, (item, row)
          assert cigar == [(u.operation, u.operation_length) for u in read.alignment.cigar], (item, row)


# ---------------------------------------------------------------- trim
@pytest.mark.parametrize('n_pairs', E.SCAN_SIZES)
def test_trim_cases_hold_the_pairs_they_promise(n_pairs):
  case, table = E.edge_trim(n_pairs), E.trim_table(n_pairs)
  assert sum(len(table.query(q0, q1)) for q0, q1, _, _, _ in case.windows) == n_pairs
  assert table.n_reads == 64 and all(31 <= r1 - r0 <= 71 for _, _, r0, r1, _ in case.windows)
  assert {m for _, _, r0, r1, m in case.windows} > {15} and all(m in (15, r1 - r0) for _, _, r0, r1, m in case.windows)
  want, kept, pair_off = E.trim_expected(n_pairs)
  assert len(kept) == n_pairs == pair_off[-1]
  # the closed form stated in csrc/trim_reads.hip, pair by pair, equals the host entry (no pair trips a check)
  host = A.trim_arrays(table, case.windows, device=False)
  TC.assert_same_arrays(host, want, case.name)
  assert 0 < kept[:STEP].sum() and len(want['cigar']) > len(want['src_row']) > 0
  if n_pairs > STEP:
    assert kept[STEP:].any()
    # pairs 1,023 and 1,024: kept and kept, and in one case kept and not kept
    edge = tuple(kept[STEP - 1:STEP + 1].tolist())
    assert edge == {1025: (True, True), 2048: (True, False), 2049: (True, True)}[n_pairs]
  if n_pairs == 2049:
    assert kept[2 * STEP - 1] and kept[2 * STEP]
  # a window whose first pair is pair 1,024 (2,048): window_row_off reads row_of exactly where a step begins
  for cut in E._TRIM_CUTS.get(n_pairs, ()):                          # pylint: disable=protected-access
    w = pair_off.index(cut)
    assert 0 < w < len(case.windows) and pair_off[w + 1] > cut and 0 < want['window_row_off'][w] < len(want['src_row'])
  if n_pairs == 2048:
    assert STEP not in pair_off                                      # ... and a case where the edge lies inside a window


# ---------------------------------------------------------------- pack
def _per_candidate(want, n_cands):
  """-> (items per candidate, list length of the candidate's items or 0)."""
  items = np.bincount(want['item_candidate'], minlength=n_cands)
  lengths = np.zeros(n_cands, np.int64)
  lengths[want['item_candidate']] = np.diff(want['item_list_off'].astype(np.int64))
  return items, lengths


@pytest.mark.parametrize('n_cands', E.SCAN_SIZES)
def test_pack_cases_hold_the_candidates_they_promise(n_cands):
  case = E.edge_pack_regions(n_cands)
  cands = E.pack_candidates(case)
  assert len(cands) == n_cands == sum(len(r.candidates) for r in case.regions)
  assert [len(r.candidates) for r in case.regions] == [n for _, n in E._PACK_LAYOUT[n_cands][0]]   # pylint: disable=protected-access
  names = [r.name[0] for r in case.regions]
  assert names[:2] == ['u', 'e'] and 's' in names
  assert not case.regions[0].sorted and case.regions[1].n_reads == 0 and case.regions[names.index('s')].sorted
  small = [r for r in case.regions if r.name[0] in 'us']
  assert all(r.n_reads == 200 for r in small)
  assert {len(c.masks) for r in small for c in r.candidates} == {0, 1, 2, 3}
  assert all(any(k == PC.GHOST for k, _ in c.support) for r in small for c in r.candidates)
  windowless = sum(not c.window for _, c in cands)
  assert n_cands // 16 < windowless < n_cands // 8
  want = E.pack_expected(n_cands, 1)
  items, lengths = _per_candidate(want, n_cands)
  assert items.sum() == len(want['item_height']) and (items == [len(c.masks) if c.window else 0 for _, c in cands]).all()
  assert items[:min(STEP, n_cands)].sum() > 0 and want['item_list_off'][items[:STEP].sum()] > 0
  first_of_region = np.cumsum([0] + [len(r.candidates) for r in case.regions]).tolist()
  if case.edge in ('inside', 'first'):
    assert items[STEP - 1] > 0 and items[STEP] > 0 and lengths[STEP - 1] >= 1 and lengths[STEP] >= 1
    assert (STEP in first_of_region) == (case.edge == 'first')
  if case.edge == 'skipped':
    # the element that makes the carry adds nothing itself; both neighbours do
    assert not cands[STEP - 1][1].window and items[STEP - 1] == 0
    assert cands[STEP][1].window and items[STEP - 2] > 0 and items[STEP] > 0
    assert lengths[STEP - 2] >= 1 and lengths[STEP] >= 1 and STEP not in first_of_region
    # the longest list lies behind the second carry: candidate 2,048, the first element of the third step
    assert want['max_list_len'] == 1025 == lengths.max() and int(np.argmax(lengths)) == 2 * STEP
    assert lengths[:2 * STEP].max() == 1024 and items[2 * STEP] == 3
  elif n_cands != 1025:
    assert want['max_list_len'] < 200


def test_the_wide_candidates_stride_the_item_loop():
  case = E.edge_pack_regions(1025)
  wide = [r for r in case.regions if r.name == 'wide']
  assert len(wide) == 1 and [len(c.masks) for c in wide[0].candidates] == list(E.WIDE_COMBOS)
  assert all(c.n_alts == 32 and all(0 < m < 1 << 32 for m in c.masks) for c in wide[0].candidates)
  host = PC.host_pack(wide[0], use_groups=True)
  assert len(host['item_height']) == sum(E.WIDE_COMBOS) and (np.diff(host['item_list_off'].astype(np.int64)) == 65).all()
  assert host['item_combo'].tolist() == [m for c in wide[0].candidates for m in c.masks]
  assert len(set(host['list_code'].tolist())) == 3


@pytest.mark.parametrize('n_cands', [1025, 2049])
def test_host_pack_equals_the_contracts_rules_on_a_sample(n_cands):
  """The checker of the GPU tests against Region.picked and the support rule of include/dvhip.h: first_alt is the
  smallest alt a row's key is listed under and group the largest; no entry: code 0, group n_alts; else code 1 if
  bit first_alt of the mask is set, else 2."""
  case = E.edge_pack_regions(n_cands)
  n_checked = 0
  for region in case.regions:
    host = PC.host_pack(region, use_groups=True)
    keys = region.keys
    off = host['item_list_off'].astype(np.int64)
    sample = set(range(0, len(region.candidates), 23)) | {len(region.candidates) - 1}
    for item, (ci, mask) in enumerate(zip(host['item_candidate'].tolist(), host['item_combo'].tolist())):
      if ci not in sample:
        continue
      cand = region.candidates[ci]
      rows = host['list_read'][off[item]:off[item + 1]].tolist()
      assert rows == region.picked(cand).tolist()
      alts_of = {}
      for key, alt in cand.support:
        alts_of.setdefault(key, []).append(alt)
      codes, groups = [], []
      for row in rows:
        alts = alts_of.get(keys[row])
        codes.append(0 if not alts else 1 if mask >> min(alts) & 1 else 2)
        groups.append(cand.n_alts if not alts else max(alts))
      assert host['list_code'][off[item]:off[item + 1]].tolist() == codes
      assert host['list_group'][off[item]:off[item + 1]].tolist() == groups
      n_checked += len(rows)
  assert n_checked > 2000


# ---------------------------------------------------------------- candidates / gVCF
@pytest.mark.parametrize('n,overflow_at', [(257, None), (300, None), (300, 260)])
def test_region_cases_hold_the_regions_they_promise(n, overflow_at):
  case = E.edge_regions(n, overflow_at)
  made = E.counters(case)
  # exactly n regions get a workgroup of the pack kernels: those plan_batch gives a slot (reads and an interval);
  # the readless ones between them come on top
  with_reads = [k for k, c in enumerate(made) if c._reads and c.interval_length() > 0]     # pylint: disable=protected-access
  assert len(with_reads) == n > E.REGION_STEP and [case.slots[k] for k in with_reads] == list(range(n))
  n_readless = case.kinds.count('readless')
  assert len(made) == len(case.spans) == n + n_readless and n_readless >= n // 4
  assert all((slot < 0) == (kind == 'readless') for slot, kind in zip(case.slots, case.kinds))
  assert [c.interval_length() for c in made] == [e - s for s, e in case.spans]
  for k, (kind, (s, e), reads) in enumerate(zip(case.kinds, case.spans, case.reads)):
    if case.slots[k] == overflow_at and kind != 'readless':
      assert kind == 'noisy' and case.slots[k] > E.REGION_STEP and len(reads) == 300 and (s, e) == (1000, 1400)
      continue
    assert kind == E.REGION_KINDS[k % 4] and e - s <= 80 and len(reads) <= 14 and (len(reads) == 0) == (kind == 'readless')
    assert all(s <= r.alignment.position.position < r.alignment.position.position + 45 <= e for r in reads)
  assert ('noisy' in case.kinds) == (overflow_at is not None)
  # the region the first step ends on and the first one behind it both have sites; every kind lies on both sides
  # of the step where the batch goes past it by more than one region
  edge = E.region_of_slot(case, E.REGION_STEP)
  assert case.kinds[E.region_of_slot(case, E.REGION_STEP - 1)] == 'snp' and case.kinds[edge] == 'indels'
  assert set(case.kinds[:edge]) >= set(E.REGION_KINDS)
  assert n == E.REGION_STEP + 1 or set(case.kinds[edge:]) >= set(E.REGION_KINDS)
  assert len({e - s for s, e in case.spans}) > 10 and len({len(r) for r in case.reads}) > 8
  assert len(E.counters(case, lo=edge)) == len(made) - edge


# ---------------------------------------------------------------- determinism
def _alt_bytes(b):
  return repr((b['items'], b['targets'], b['starts'], [(r.fragment_name, r.aligned_sequence, r.aligned_quality,
                                                      r.alignment.position.position) for r in b['reads']])).encode()


def _pack_bytes(case):
  inputs = PC.DeviceInputs(list(case.regions))
  return b''.join([inputs.read_pos.tobytes(), inputs.read_end.tobytes(), inputs.read_key.tobytes(), inputs.masks.tobytes(),
                   inputs.support_key.tobytes(), inputs.support_alt.tobytes(), bytes(inputs.slices), bytes(inputs.cands)])


def _regions_bytes(case):
  return repr((case.ref.seq, case.spans, case.kinds, [[(r.fragment_name, r.aligned_sequence, r.alignment.position.position,
                                                       [(u.operation, u.operation_length) for u in r.alignment.cigar])
                                                      for r in reads] for reads in case.reads])).encode()


def test_two_builds_give_equal_bytes():
  first = _alt_bytes(E.edge_alt_align(2049))
  E._alt_align_stream.cache_clear()                                  # pylint: disable=protected-access
  assert _alt_bytes(E.edge_alt_align.__wrapped__(2049)) == first
  table = E.trim_table(2049)
  again = E._trim_reads.__wrapped__()[1]                             # pylint: disable=protected-access
  for name in ('read_pos', 'read_seq_off', 'read_cigar_off', 'cigar', 'bases', 'quals', 'read_end'):
    assert getattr(table, name).tobytes() == getattr(again, name).tobytes(), name
  assert E.edge_trim.__wrapped__(2049).windows == E.edge_trim(2049).windows
  assert _pack_bytes(E.edge_pack_regions.__wrapped__(2049)) == _pack_bytes(E.edge_pack_regions(2049))
  assert _pack_bytes(E.edge_pack_regions.__wrapped__(1025)) == _pack_bytes(E.edge_pack_regions(1025))
  assert _regions_bytes(E.edge_regions.__wrapped__(300, 260)) == _regions_bytes(E.edge_regions(300, 260))
