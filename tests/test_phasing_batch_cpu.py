"""dv_phase_reads_batch (csrc/phasing.hip's host code: the checker in a loop over regions given as arrays) against
dv_phase_reads region by region, the plan's "outside the device limits" count, and the argument errors.  Host only."""
import ctypes as C

import numpy as np
import pytest

from tests import phasing_cases as pc
from deepvariant_amd import _lib
from deepvariant_amd import direct_phasing as dp


def check_batch(cases, min_alleles_to_phase, on_host=0):
  got, stats = pc.run_batch(cases, min_alleles_to_phase, device=False)
  assert len(got) == len(cases)
  for case, g in zip(cases, got):
    assert pc.same(g, pc.reference(case, min_alleles_to_phase)), case['name']
  assert stats['regions'] == len(cases)
  assert stats['regions_on_host'] == on_host
  assert stats['launches'] == 0 and stats['combinations'] == 0
  return stats


@pytest.mark.parametrize('min_alleles_to_phase', [1, 2])
def test_reference_vectors_as_a_batch(min_alleles_to_phase):
  vectors = pc.vector_cases()
  cases = vectors[:5] + [pc.EMPTY] + vectors[5:11] + [pc.NO_CANDIDATES] + vectors[11:]
  stats = check_batch(cases, min_alleles_to_phase)
  assert stats['sites_in_graphs'] > 0 and stats['vertices'] >= 2 * stats['sites_in_graphs'] - 4


def test_vectors_keep_their_known_answers():
  by_name = {c['name']: c for c in pc.vector_cases()}
  got, _ = pc.run_batch([by_name['simple'], by_name['broken_path'], by_name['two_blocks_with_score_tie']], 2, device=False)
  assert got[0][0].tolist() == [1, 1, 1, 2, 2]
  assert got[1][0].tolist() == [0, 0, 0, 2, 2, 1, 1]
  assert got[2][0].tolist() == [1, 1, 2, 2] + [0] * 8
  assert got[2][1].tolist() == [1, 2, 1, 2, 0, 0] and got[2][2][:4].tolist() == [1, 1, 0, 0]


@pytest.mark.parametrize('min_alleles_to_phase', [1, 2])
def test_generated_regions(min_alleles_to_phase):
  cases = pc.generated_cases(200)
  check_batch(cases, min_alleles_to_phase)
  # the generator reaches what it is meant to reach
  kinds = {'indel': 0, 'ref2': 0, 'ref3': 0, 'g_ref_t': 0, 'unknown_read': 0, 'low_quality': 0, 'phased': 0}
  for case in cases:
    for start, end, entries in case['sites']:
      texts = [t for t, is_ref, _ in entries if not is_ref]
      kinds['indel'] += any(len(t) != end - start for t in texts)
      for text, is_ref, infos in entries:
        kinds['ref2'] += is_ref and len(infos) == 2
        kinds['ref3'] += is_ref and len(infos) == 3
        kinds['g_ref_t'] += is_ref and len(infos) >= 3 and 'G' in texts and 'T' in texts
        kinds['unknown_read'] += any(r < 0 for r, _ in infos)
        kinds['low_quality'] += any(q for _, q in infos)
    kinds['phased'] += bool(np.any(pc.reference(case, min_alleles_to_phase)[0] > 0))
  assert all(n >= 5 for n in kinds.values()), kinds
  assert kinds['phased'] >= 100


def test_case_lists_keep_their_lengths():
  """Other tests slice these lists and pin the generated regions: new cases go into lists of their own."""
  assert len(pc.vector_cases()) == 19 and len(pc.named_cases()) == 8 and len(pc.generated_cases(200)) == 200
  assert len(pc.at_limit_cases()) == 2 and len(pc.over_limit_cases()) == 4 and len(pc.edge_cases()) == 5
  assert pc.generated_case(3) == pc.generated_cases(4)[3] and pc.dense_case(5) == pc.dense_cases(6)[5]
  assert [c['n_reads'] for c in pc.dense_cases(21)] == list(pc.DENSE_READ_COUNTS)


@pytest.mark.parametrize('min_alleles_to_phase', [1, 2, 3])
def test_dense_regions(min_alleles_to_phase):
  cases = pc.dense_cases(126)
  check_batch(cases, min_alleles_to_phase)           # regions_on_host == 0: all of them are the device's
  # the generator reaches what it is for
  words, site_sizes = {}, {}
  both_phases = blocks = 0
  for case in cases:
    n_words = (case['n_reads'] + 63) // 64
    words[n_words] = words.get(n_words, 0) + 1
    for size in {len(entries) for _, _, entries in case['sites']}:
      site_sizes[size] = site_sizes.get(size, 0) + 1
    assert max(len(entries) for _, _, entries in case['sites']) <= pc.MAX_VERTICES
    phases, _, flags = pc.reference(case, min_alleles_to_phase)
    both_phases += {1, 2} <= set(phases.tolist())
    at = np.cumsum([0] + [len(entries) for _, _, entries in case['sites']])
    blocks += sum(bool(flags[a:b].any()) for a, b in zip(at[:-1], at[1:])) >= 2
  print('words per read set -> cases:', dict(sorted(words.items())))
  print('entries per site -> cases:', dict(sorted(site_sizes.items())))
  print('cases with both phases: %d, with two or more first-in-block allele pairs: %d' % (both_phases, blocks))
  assert all(words.get(n, 0) >= 5 for n in (1, 2, 3, 4, 5, 8, 9, 12, 16)), words
  assert site_sizes.get(8, 0) >= 15 and all(site_sizes.get(n, 0) >= 10 for n in (5, 6, 7)), site_sizes
  assert both_phases >= 100 and blocks >= 40


def test_edge_cases():
  cases = pc.edge_cases()
  for m in (1, 2, 3):
    check_batch(cases, m)
  by_name = {c['name']: c for c in cases}
  # what the names promise, in the checker's own answer
  phases, allele_phases, _ = pc.reference(by_name['deep_and_long'], 1)
  assert set(phases[0::2].tolist()) | set(phases[1::2].tolist()) == {1, 2} and len(set(phases[0::2].tolist())) == 1
  assert len(set(phases[1::2].tolist())) == 1 and (len(by_name['deep_and_long']['sites']) - 1) * pc.MAX_READS > 1 << 16
  for name in ('vertex_all_low_quality_middle', 'vertex_all_low_quality_first'):
    phases, allele_phases, _ = pc.reference(by_name[name], 1)
    assert (allele_phases >= 0).all(), name             # the vertex without reads is a vertex all the same
    assert phases[3] != 0 and phases[3] == phases[4] == phases[5], name
    assert phases[0] == phases[1] == phases[2] and phases[0] not in (0, phases[3]), name
  phases, allele_phases, _ = pc.reference(by_name['ref_vertex_of_unknown_reads'], 1)
  assert allele_phases[0] >= 0 and allele_phases[3] >= 0             # REF is in the graph at both sites
  assert phases[0] == phases[1] == phases[2] != 0 and phases[3] == phases[4] == phases[5] not in (0, phases[0])
  phases, allele_phases, _ = pc.reference(by_name['single_vertex_sites'], 1)
  assert allele_phases.tolist()[0] >= 0 and allele_phases.tolist()[3] >= 0 and set(phases.tolist()) >= {1, 2}


def test_named_cases():
  check_batch(pc.named_cases(), 1)
  check_batch(pc.named_cases(), 2)
  by_name = {c['name']: c for c in pc.named_cases()}
  # what the names promise, in the checker's own answer
  phases, allele_phases, flags = pc.reference(by_name['restart_in_the_middle'], 1)
  assert flags.tolist() == [0, 0, 0, 0, 1, 1, 0, 0] or flags.sum() >= 2      # a block starts past the first site
  assert phases[4] != 0 and phases[4] == phases[5] == phases[8] and phases[6] == phases[7] == phases[9] != phases[4]
  phases, allele_phases, _ = pc.reference(by_name['reads_130'], 1)
  assert set(phases[0::2].tolist()) | set(phases[1::2].tolist()) == {1, 2} and len(set(phases[0::2].tolist())) == 1
  phases, allele_phases, _ = pc.reference(by_name['ref_between_g_and_t'], 1)
  assert allele_phases[3] == -1                       # two reference reads: REF is no vertex at the second site


def test_limit_stat():
  check_batch(pc.at_limit_cases(), 1)
  over = pc.over_limit_cases()
  check_batch(over, 1, on_host=len(over))
  mixed = pc.named_cases()[:2] + over[:1] + pc.generated_cases(5) + over[2:3]
  check_batch(mixed, 2, on_host=2)


def test_regions_do_not_depend_on_their_neighbours():
  cases = pc.generated_cases(20) + pc.named_cases()
  forward, _ = pc.run_batch(cases, 1, device=False)
  backward, _ = pc.run_batch(cases[::-1], 1, device=False)
  for f, b in zip(forward, backward[::-1]):
    assert pc.same(f, b)


# ---- errors: the return code, dv_last_error, outputs untouched

def call(regions_of=None, device=False, **patch):
  """dv_phase_reads_batch on two good regions, with arguments replaced by name -> (status, outputs)."""
  cases = regions_of or [pc.vector_cases()[2], pc.vector_cases()[3]]
  table, cands, alleles, bases, support, low, n_reads = dp.concat_regions([pc.region_arrays(c) for c in cases])
  for field, (k, value) in patch.pop('region', {}).items():
    table[field][k] = value
  for field, (k, value) in patch.pop('candidate', {}).items():
    cands[field][k] = value
  for field, (k, value) in patch.pop('allele', {}).items():
    alleles[field][k] = value
  phases = np.full(n_reads, 77, np.int32)
  allele_phases = np.full(len(alleles), 77, np.int32)
  flags = np.full(len(alleles), 77, np.uint8)
  args = {'regions': table.ctypes.data, 'n_regions': len(table), 'candidates': cands.ctypes.data,
          'n_candidates': len(cands), 'alleles': alleles.ctypes.data, 'n_alleles': len(alleles),
          'bases': bases.ctypes.data, 'n_bases': len(bases), 'support_reads': support.ctypes.data,
          'support_low_quality': low.ctypes.data, 'n_support': len(support), 'n_reads_total': n_reads,
          'min_alleles_to_phase': 1, 'read_phases': phases.ctypes.data, 'allele_phases': allele_phases.ctypes.data,
          'allele_flags': flags.ctypes.data, 'stats': None}
  args.update(patch)
  fn = _lib.lib().dv_phase_reads_batch_device if device else _lib.lib().dv_phase_reads_batch
  status = fn(*(list(args.values()) + ([None] if device else [])))
  untouched = bool(np.all(phases == 77) and np.all(allele_phases == 77) and np.all(flags == 77))
  return status, untouched, _lib.lib().dv_last_error().decode()


def test_good_call_of_the_error_harness():
  status, untouched, _ = call()
  assert status == _lib.DV_OK and not untouched


@pytest.mark.parametrize('name', ['regions', 'candidates', 'alleles', 'bases', 'support_reads', 'support_low_quality',
                                  'read_phases'])
def test_null_pointer(name):
  status, untouched, message = call(**{name: None})
  assert status == _lib.DV_ERR_INVALID_ARGUMENT and untouched and 'dv_phase_reads_batch' in message


@pytest.mark.parametrize('name', ['n_regions', 'n_candidates', 'n_alleles', 'n_bases', 'n_support', 'n_reads_total'])
def test_negative_count(name):
  status, untouched, message = call(**{name: -1})
  assert status == _lib.DV_ERR_INVALID_ARGUMENT and untouched and message


@pytest.mark.parametrize('patch', [
    {'region': {'candidate_off': (1, 6)}}, {'region': {'n_candidates': (1, 99)}}, {'region': {'candidate_off': (0, -1)}},
    {'region': {'allele_off': (1, 1000)}}, {'region': {'n_alleles': (0, -2)}},
    {'region': {'support_off': (1, 1 << 40)}}, {'region': {'n_support': (1, 1 << 62)}},
    {'region': {'n_reads': (1, 6)}}, {'region': {'first_read': (0, -1)}}, {'region': {'n_reads': (0, -1)}},
    {'candidate': {'allele_off': (0, 100)}}, {'candidate': {'n_alleles': (6, 3)}}, {'candidate': {'n_alleles': (0, -1)}},
    {'candidate': {'allele_off': (3, 0)}},                       # into the other region's alleles
    {'allele': {'bases_off': (0, 1 << 33)}}, {'allele': {'bases_len': (1, -1)}}, {'allele': {'support_off': (0, -1)}},
    {'allele': {'n_support': (11, 100)}}, {'allele': {'support_off': (6, 0)}},     # into the other region's support
    {'n_candidates': 5}, {'n_alleles': 3}, {'n_support': 4}, {'n_reads_total': 9}, {'n_bases': 2},
])
def test_slices_outside_their_tables(patch):
  status, untouched, message = call(**patch)
  assert status == _lib.DV_ERR_INVALID_ARGUMENT and untouched and message


def test_unordered_candidates_name_the_smallest_region():
  good = pc.vector_cases()[2]
  status, untouched, message = call(regions_of=[good, pc.UNORDERED, good, pc.UNORDERED])
  assert status == _lib.DV_ERR_BAD_INPUT and untouched
  assert 'region 1:' in message and 'Check failed: candidates[i - 1].variant().start() < candidate.variant().start()' in message
  status, untouched, message = call(regions_of=[good], candidate={'start': (1, 100)})      # equal starts
  assert status == _lib.DV_ERR_BAD_INPUT and untouched and 'region 0:' in message


def test_read_index_past_the_regions_reads():
  status, untouched, message = call(region={'n_reads': (0, 4)})
  assert status == _lib.DV_ERR_BAD_INPUT and untouched and 'region 0:' in message


def test_device_entry_refuses_the_same_before_any_device_work():
  """Argument checks come before the device is looked for: they hold on a machine without one."""
  status, untouched, message = call(device=True, regions=None)
  assert status == _lib.DV_ERR_INVALID_ARGUMENT and untouched and 'dv_phase_reads_batch_device' in message
  status, untouched, _ = call(device=True, regions_of=[pc.vector_cases()[2], pc.UNORDERED])
  assert status == _lib.DV_ERR_BAD_INPUT and untouched


def test_nothing_to_phase_needs_no_device():
  for cases in ([], [pc.EMPTY], [pc.NO_CANDIDATES, pc.EMPTY]):
    got, stats = pc.run_batch(cases, 1, device=True)
    assert stats['launches'] == 0 and stats['regions'] == len(cases)
    for case, g in zip(cases, got):
      assert g[0].tolist() == [0] * case['n_reads']
  last = _lib.DvPhasingStats()
  assert _lib.lib().dv_phase_device_last_stats(C.addressof(last)) == _lib.DV_OK
  assert last.regions == 2 and last.launches == 0
  assert _lib.lib().dv_phase_device_last_stats(None) == _lib.DV_ERR_INVALID_ARGUMENT


# ---- AlleleCounter.phasing_arrays' pure array step against the lists DirectPhasing.phase builds

class _Call:
  def key(self):
    return ('test',)


def _synthetic_counter(seed):
  """An AlleleCounter as the device candidate pass would leave it (events, sites, selected alleles, words), made by
  hand: substitutions, insertions, deletions, uncalled and REFERENCE events, low-quality ones, two rows that share a
  read key (the earlier one's events are "overwritten" where both have one)."""
  import types
  from deepvariant_amd import allelecounter as ac
  rng = np.random.RandomState(seed)
  n_rows, seq_len, start, w0 = int(rng.randint(6, 30)), 40, 1000, 990
  window = bytes(rng.choice(list(b'ACGT'), 400).astype(np.uint8))
  bases = rng.choice(list(b'ACGT'), n_rows * seq_len).astype(np.uint8)
  seq_off = (np.arange(n_rows + 1) * seq_len).astype(np.uint32)
  keys = ['read%d/0' % r for r in range(n_rows)]
  if seed % 2:
    keys[n_rows - 2] = keys[1]                                    # supplementary alignment: one key, two rows
  key_of = {k: i for i, k in enumerate(dict.fromkeys(keys))}
  offsets = np.sort(rng.choice(np.arange(5, 200), int(rng.randint(2, 9)), replace=False))
  sites, alleles, events, words = [], [], [], []
  for offset in offsets.tolist():
    selected = []                                                 # (type, length, row, read_offset)
    for base in rng.permutation(list(b'ACGT'))[:int(rng.randint(1, 3))].tolist():
      row, ro = int(rng.randint(n_rows)), int(rng.randint(1, seq_len - 8))
      bases[row * seq_len + ro] = base
      selected.append((ac.SUBSTITUTION, 1, row, ro))
    if rng.rand() < 0.3:
      selected.append((ac.INSERTION, int(rng.randint(1, 4)), int(rng.randint(n_rows)), int(rng.randint(1, seq_len - 8))))
    if rng.rand() < 0.3:
      selected.append((ac.DELETION, int(rng.randint(1, 4)), int(rng.randint(n_rows)), int(rng.randint(1, seq_len - 8))))
    if rng.rand() < 0.15:
      selected = [s for s in selected if s[0] == ac.SUBSTITUTION][:1] + [(ac.DELETION, 2, 0, 3)]
    order = rng.permutation(len(selected)).tolist()               # the device's ordinals are in no text order
    selected = [selected[i] for i in order]
    sites.append((offset, 3, 20, len(alleles), len(selected)))
    alleles += [(length | (kind << 28), 5, row, ro) for kind, length, row, ro in selected]
    rows = rng.permutation(n_rows)[:int(rng.randint(2, n_rows + 1))].tolist()
    site_events = []
    for row in rows:
      what = rng.rand()
      low = int(rng.rand() < 0.1)
      if what < 0.3:
        site_events.append((row, ac.REFERENCE, 1, low, ac.EVENT_UNCALLED))
      elif what < 0.4:
        site_events.append((row, ac.SUBSTITUTION, 1, low, ac.EVENT_UNCALLED))
      else:
        w = int(rng.randint(len(selected)))
        if selected[w][0] == ac.DELETION and rng.rand() < 0.7:      # sometimes a selected allele without support
          w = 0
        site_events.append((row, selected[w][0], selected[w][1], low, w))
    last = {}
    for k, ev in enumerate(site_events):
      last[keys[ev[0]]] = k
    for k, (row, kind, length, low, w) in enumerate(site_events):
      events.append((offset, row, 5, length | (kind << 28) | (low << 31)))
      words.append(w if last[keys[row]] == k else ac.EVENT_OVERWRITTEN)
  counter = ac.AlleleCounter(None, 'chr1', start, start + 300, track_ref_reads=True)
  table = types.SimpleNamespace(keys=keys, bases=bases, read_seq_off=seq_off, n_reads=n_rows)
  counter._events = np.array(events, ac._EVENT_DTYPE)                       # pylint: disable=protected-access
  counter._event_ctx = (table, window, w0)                                  # pylint: disable=protected-access
  counter._interval_ref = window[start - w0:start - w0 + 300].decode()      # pylint: disable=protected-access
  counter._cand = (_Call().key(), np.array(sites, ac.CANDIDATE_SITE_DTYPE),  # pylint: disable=protected-access
                   np.array(alleles, ac.CANDIDATE_ALLELE_DTYPE), np.array(words, np.int32))
  return counter, keys, key_of


def _lists_of_the_object_route(counter, keys):
  """The calls as process() builds them and the lists DirectPhasing.phase makes of them."""
  from deepvariant_amd import variant_calling
  caller = variant_calling.VariantCaller(variant_calling.VariantCallerOptions(2, 2, 0.1, 0.1, sample_name='s',
                                                                              track_ref_reads=True))
  calls = [caller._call_with_alt_alleles(site, site.selected, site.total)    # pylint: disable=protected-access
           for site in counter.candidates(_Call())]
  index = {key: i for i, key in enumerate(keys)}                  # a later duplicate wins
  out = []
  for cand in calls:
    entries = []
    if cand.ref_support_ext:
      entries.append(('', True, cand.ref_support_ext))
    for allele, infos in cand.allele_support_ext.items():
      if allele != dp.K_UNCALLED_ALLELE:
        entries.append((allele, False, infos))
    out.append((cand.variant.start, cand.variant.end,
                [(allele, is_ref, [(index.get(i.read_name, -1), bool(i.is_low_quality)) for i in infos])
                 for allele, is_ref, infos in entries]))
  return out


@pytest.mark.parametrize('seed', range(40))
def test_phasing_arrays_pure_step(seed):
  counter, keys, _ = _synthetic_counter(seed)
  want = _lists_of_the_object_route(counter, keys)
  cands, alleles, bases, support, low = counter.phasing_arrays(_Call())
  assert len(cands) == len(want) and cands['start'].tolist() == [w[0] for w in want]
  assert cands['end'].tolist() == [w[1] for w in want]
  blob = bytes(bases)
  for c, (start, end, entries) in zip(cands, want):
    got = alleles[c['allele_off']:c['allele_off'] + c['n_alleles']]
    assert len(got) == len(entries)
    substitutions = all(is_ref or len(text) == end - start for text, is_ref, _ in entries)
    for a, (text, is_ref, infos) in zip(got, entries):
      assert bool(a['is_ref']) == is_ref and a['bases_len'] == len(text)
      if substitutions:                                           # bytes matter only where the filter lets the site in
        assert blob[a['bases_off']:a['bases_off'] + a['bases_len']] == text.encode()
      s = slice(int(a['support_off']), int(a['support_off']) + int(a['n_support']))
      assert list(zip(support[s].tolist(), [bool(q) for q in low[s].tolist()])) == infos
  # and the phases are the ones the lists give
  case = {'name': 'lists', 'n_reads': len(keys), 'sites': want}
  got = dp.phase_arrays([(cands, alleles, bases, support, low, len(keys))], 1, device=False)
  assert pc.same(got[0], pc.reference(case, 1))
