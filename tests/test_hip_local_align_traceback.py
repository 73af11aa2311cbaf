"""The banded trace-back of dv_local_align_pairs_device on the device (csrc/local_align.hip: trace_back, in the
same launch as the sweeps; DV_REALIGN_DEVICE_TRACEBACK=1) against dv_local_align, pair by pair: every field
and the CIGAR text.

The kernel hands a pair back to the host's banded_cigar when its band would pass DV_LOCAL_ALIGN_DEVICE_MAX_BAND or
its runs do not fit DV_LOCAL_ALIGN_DEVICE_MAX_RUNS, and the host would produce the right CIGAR for any pair the
kernel hands back.  So every check here also pins the split: dv_local_align_band gives each pair's final band and
run count on the host, traced_on_host must be exactly the number of pairs past one of the two limits, and
traced_on_device all the others.  A kernel that gave up on a pair it should have traced fails that count; one that
traced a pair wrongly fails the comparison.
"""
import os

import numpy as np
import pytest

from deepvariant_amd import _lib
from deepvariant_amd import fast_pass_aligner as F

pytestmark = pytest.mark.gpu

LETTERS = np.array(list('ACGT'))
DEFAULT = (2, 2, 3, 1)
REALIGNER = (4, 6, 8, 1)
MAX_BAND = _lib.DV_LOCAL_ALIGN_DEVICE_MAX_BAND
MAX_RUNS = _lib.DV_LOCAL_ALIGN_DEVICE_MAX_RUNS
SWITCH = 'DV_REALIGN_DEVICE_TRACEBACK'


def _fields(a):
  return (a.score, a.ref_begin, a.ref_end, a.query_begin, a.query_end, a.mismatches, bytes(a.cigar))


def _host(reference, query, scoring):
  """dv_local_align, or None where it refuses (an empty sequence)."""
  try:
    return _fields(F.local_align(reference, query, *scoring))
  except _lib.DvError:
    return None


def _on_device(reference, query):
  return (reference and query and len(query) <= _lib.DV_LOCAL_ALIGN_DEVICE_MAX_QUERY and
          len(reference) <= _lib.DV_LOCAL_ALIGN_DEVICE_MAX_REFERENCE)


def _check(sequences, pairs, scoring, traceback=True):
  """One device call over `pairs` with the trace-back on (or off); every result against the host aligner, and
  the device / host split of the trace-backs against dv_local_align_band.  -> (results, stats, trace-back stats,
  [(band, runs)] of the pairs that hold an alignment)"""
  before = os.environ.get(SWITCH)
  os.environ[SWITCH] = '1' if traceback else '0'
  try:
    got, stats, tb = F.local_align_pairs_device(sequences, pairs, scoring, with_stats=True, with_traceback_stats=True)
  finally:
    if before is None:
      del os.environ[SWITCH]
    else:
      os.environ[SWITCH] = before
  assert len(got) == len(pairs)
  shapes = []
  for (r, q), g in zip(pairs, got):
    want = _host(sequences[r], sequences[q], scoring)
    assert (None if g is None else _fields(g)) == want, (len(sequences[r]), len(sequences[q]), scoring,
                                                        sequences[r][:80], sequences[q][:80])
    if want is not None and want[0] > 0 and _on_device(sequences[r], sequences[q]):
      band, runs = F.local_align_band(sequences[r], sequences[q], *scoring)
      assert band >= 1 and runs >= 1
      shapes.append((band, runs))
  on_host = sum(1 for band, runs in shapes if band > MAX_BAND or runs > MAX_RUNS)
  if traceback:
    assert (tb.traced_on_device, tb.traced_on_host) == (len(shapes) - on_host, on_host), shapes
    kept = [band for band, runs in shapes if band <= MAX_BAND and runs <= MAX_RUNS]
    assert tb.widest_band == (max(kept) if kept else 0)
    assert (tb.band_cells > 0) == bool(kept)
  else:
    assert (tb.traced_on_device, tb.traced_on_host, tb.band_cells, tb.widest_band) == (0, len(shapes), 0, 0)
  assert stats.pairs == len(pairs)
  swept = sum(1 for r, q in pairs if _on_device(sequences[r], sequences[q]))
  assert stats.launches == (1 if swept else 0)
  return got, stats, tb, shapes


def _random(rng, n):
  return ''.join(rng.choice(LETTERS, size=n))


def _mutated(rng, piece, edits):
  piece = list(piece)
  for _ in range(edits):
    if not piece:
      break
    k = int(rng.integers(0, len(piece)))
    kind = int(rng.integers(0, 4))
    if kind == 0:
      piece[k] = str(rng.choice(LETTERS))
    elif kind == 1:
      piece[k:k] = list(rng.choice(LETTERS, size=int(rng.integers(1, 12))))
    elif kind == 2:
      del piece[k:k + int(rng.integers(1, 12))]
    else:
      piece[k] = 'N'
  return ''.join(piece)


def _other(base):
  return 'ACGT'[('ACGT'.index(base) + 1) % 4]


def test_smallest_problems():
  """Sub-problems of one and two query bases and of one reference base (a q_len == 1 problem never enters the walk
  and is 1M), a query equal to its reference (band 1), and lengths on both sides of the 64 lanes."""
  rng = np.random.default_rng(31)
  reference = _random(rng, 300)
  sequences = [reference, 'G', 'GT', 'T', reference[40:42], 'C' + reference[100] + 'C' if reference[100] != 'C' else 'AGA',
               reference[10] + _other(reference[11]), 'AC', 'CA']
  pairs = [(0, k) for k in range(1, len(sequences))] + [(1, 0), (2, 0), (3, 3), (7, 8), (8, 7), (2, 2), (1, 2), (2, 1)]
  for n in (63, 64, 65, 150):
    copy = reference[20:20 + n]
    edited = _mutated(rng, copy, 3)
    sequences += [copy, edited]
    pairs += [(0, len(sequences) - 2), (len(sequences) - 2, len(sequences) - 2), (0, len(sequences) - 1),
              (len(sequences) - 2, len(sequences) - 1), (len(sequences) - 1, len(sequences) - 2)]
  for scoring in (REALIGNER, DEFAULT):
    _, _, tb, shapes = _check(sequences, pairs, scoring)
    assert (1, 1) in shapes and tb.traced_on_device > 0


def _indel_pairs(rng):
  """One reference; reads with a single deletion or insertion of MAX_BAND - 1, MAX_BAND and MAX_BAND + 1 bases (the
  band starts at the cap, one past it and two past it), and the read whose band has to double from 1 to 8."""
  reference = _random(rng, 700)
  sequences, pairs = [reference], []
  for size in (MAX_BAND - 1, MAX_BAND, MAX_BAND + 1):
    sequences.append(reference[100:250] + reference[250 + size:400 + size])                  # a deletion
    sequences.append(reference[100:250] + _random(rng, size) + reference[250:400])          # an insertion
  sequences.append(reference[100:170] + 'ACCAT' + reference[170:230] + reference[235:300])   # 5I ... 5D: band 1 -> 8
  pairs = [(0, k) for k in range(1, len(sequences))]
  return sequences, pairs


def test_the_band_schedule():
  rng = np.random.default_rng(37)
  sequences, pairs = _indel_pairs(rng)
  _, _, tb, shapes = _check(sequences, pairs, REALIGNER)
  # what the generator is for (the split itself is checked against dv_local_align_band in _check)
  assert sorted(band for band, _ in shapes) == [8, MAX_BAND, MAX_BAND, MAX_BAND + 1, MAX_BAND + 1, MAX_BAND + 2,
                                                MAX_BAND + 2]
  assert (tb.traced_on_device, tb.traced_on_host, tb.widest_band) == (3, 4, MAX_BAND)
  _check(sequences, pairs, DEFAULT)


def _edited_read(reference, start, n_edits, alternate):
  """reference[start:] with n_edits single-base edits 20 bases apart: deletions, or deletions and insertions in
  turn (then the two sides stay within a base of each other and the band stays narrow)."""
  out, at = [], start
  for e in range(n_edits):
    out.append(reference[at:at + 20])
    at += 20
    if alternate and e % 2:
      out.append(_other(reference[at]))       # an inserted base that differs from the next reference base
    else:
      at += 1                                 # a deleted base
  out.append(reference[at:at + 20])
  return ''.join(out)


def test_the_run_cap():
  """2n + 1 runs for n single-base edits.  With deletions alone the band (n + 1) passes its cap before the runs
  pass theirs; edits that alternate between deletion and insertion keep the band narrow, so that read reaches the
  kernel's own run count."""
  rng = np.random.default_rng(41)
  reference = _random(rng, 900)
  many, fewer = MAX_RUNS // 2 + 1, MAX_BAND - 1
  sequences = [reference,
               _edited_read(reference, 30, many, False),            # 2 * 33 + 1 runs: to the host
               _edited_read(reference, 30, fewer, False),           # 61 runs, band 31: stays
               _edited_read(reference, 30, many, True),             # 67 runs in a narrow band: to the host
               _edited_read(reference, 30, many - 1, True),         # 65 runs: to the host
               _edited_read(reference, 30, many - 2, True)]         # 63 runs: stays
  pairs = [(0, k) for k in range(1, len(sequences))]
  _, _, tb, shapes = _check(sequences, pairs, REALIGNER)
  assert [runs for _, runs in shapes] == [2 * many + 1, 2 * fewer + 1, 2 * many + 1, 2 * many - 1, 2 * many - 3]
  assert shapes[0][0] == many + 1 and shapes[1][0] == MAX_BAND
  assert all(band <= 4 for band, _ in shapes[2:])                   # the run cap alone decides these three
  assert (tb.traced_on_device, tb.traced_on_host) == (2, 3)


def test_ties():
  """The homopolymers, tandem repeats and the query that occurs twice of
  test_hip_local_align.py::test_ties_go_to_the_first_column_and_the_smallest_row: every tie rule of the
  trace-back (diagonal before a gap, extension before opening, deletion before insertion) decides these CIGARs."""
  rng = np.random.default_rng(7)
  unit = _random(rng, 40)
  twice = _random(rng, 30) + unit + _random(rng, 25) + unit + _random(rng, 10)
  same = _random(rng, 300)
  sequences = ['A' * 50, 'A' * 20, 'A' * 200, 'A' * 130,          # homopolymers, both ways round
               same,                                               # a query equal to its reference
               twice, unit,                                        # a query that occurs twice
               'TGA' * 30, 'TGA' * 10, 'AC' * 100, 'AC' * 70 + 'CA' * 20, 'ACGGT' * 40, 'GGTAC' * 13,   # tandem repeats
               unit + unit + unit]
  pairs = [(0, 1), (1, 0), (2, 3), (3, 2), (0, 0), (4, 4), (5, 6), (6, 5), (7, 8), (8, 7), (9, 10), (10, 9),
           (11, 12), (12, 11), (13, 6), (6, 13), (13, 13)]
  for scoring in (REALIGNER, DEFAULT, (1, 1, 1, 1)):
    _, _, tb, _ = _check(sequences, pairs, scoring)
    assert tb.traced_on_device > 0


def _fuzz_batch(seed):
  """The generator of test_hip_local_align.py::test_mutated_pieces_junk_repeats_and_n_runs."""
  rng = np.random.default_rng(seed)
  reference = ''.join(rng.choice(LETTERS, size=700))
  reference = reference[:300] + 'TGA' * 15 + reference[300:500] + 'N' * 3 + reference[500:]
  queries = []
  for _ in range(75):
    a = int(rng.integers(0, len(reference) - 50))
    piece = list(reference[a:a + int(rng.integers(20, 400))])
    for _ in range(int(rng.integers(0, 6))):
      k = int(rng.integers(0, len(piece)))
      kind = int(rng.integers(0, 4))
      if kind == 0:
        piece[k] = str(rng.choice(LETTERS))
      elif kind == 1:
        piece[k:k] = list(rng.choice(LETTERS, size=int(rng.integers(1, 12))))
      elif kind == 2:
        del piece[k:k + int(rng.integers(1, 12))]
      else:
        piece[k] = 'N'
    clip = ''.join(rng.choice(LETTERS, size=int(rng.integers(0, 10))))
    queries.append(clip + ''.join(piece) + clip[::-1])
  queries += [''.join(rng.choice(LETTERS, size=30)), 'A', 'TGA' * 20, 'N' * 10, reference, reference[100:140].lower()]
  sequences = [reference] + queries
  return sequences, [(0, k) for k in range(1, len(sequences))]


@pytest.mark.parametrize('seed,scoring', [(1, (4, 6, 8, 2)), (2, (2, 2, 3, 1)), (3, (1, 4, 6, 1)), (4, (4, 6, 8, 1))])
def test_mutated_pieces_junk_repeats_and_n_runs(seed, scoring):
  sequences, pairs = _fuzz_batch(seed)
  _, _, tb, shapes = _check(sequences, pairs, scoring)
  assert tb.traced_on_device > 50 and len({band for band, _ in shapes}) > 3     # many bands, most of them traced
  _check(sequences, [(0, 1)], scoring)                                          # and a batch of one


def test_the_longest_query():
  """2,048 bases with three small edits (3D, 7I, 1X: the two sides differ by 4, band 5) against 2,100: the largest
  scratch area and the longest walk."""
  rng = np.random.default_rng(43)
  reference = _random(rng, 2100)
  piece = reference[20:700] + reference[703:1400] + 'GATTACA' + reference[1400:1900] + _other(reference[1900]) + reference[1901:]
  query = piece[:_lib.DV_LOCAL_ALIGN_DEVICE_MAX_QUERY]
  assert len(query) == _lib.DV_LOCAL_ALIGN_DEVICE_MAX_QUERY
  got, _, tb, shapes = _check([reference, query], [(0, 1)], REALIGNER)
  assert shapes == [(5, 5)] and (tb.traced_on_device, tb.widest_band) == (1, 5)
  assert got[0].query_begin == 0 and got[0].query_end == len(query) - 1
  assert tb.band_cells == len(query) * (2 * 5 + 1)


def test_switched_off_every_cigar_comes_from_the_host():
  sequences, pairs = _fuzz_batch(4)
  on, _, tb_on, _ = _check(sequences, pairs, REALIGNER)
  off, _, tb_off, _ = _check(sequences, pairs, REALIGNER, traceback=False)
  assert tb_off.traced_on_device == 0 and tb_off.traced_on_host == tb_on.traced_on_device + tb_on.traced_on_host
  assert [None if a is None else _fields(a) for a in on] == [None if a is None else _fields(a) for a in off]


def test_three_hundred_pairs_in_one_launch():
  """The 300-pair batch of test_hip_local_align.py::test_batch_sizes."""
  n_pairs = 300
  rng = np.random.default_rng(100 + n_pairs)
  references = [_random(rng, int(rng.integers(200, 500))) for _ in range(min(n_pairs, 7))]
  sequences, pairs = list(references), []
  for k in range(n_pairs):
    r = k % len(references)
    a = int(rng.integers(0, len(references[r]) - 150))
    sequences.append(_mutated(rng, references[r][a:a + int(rng.integers(30, 151))], int(rng.integers(0, 5))))
    pairs.append((r, len(sequences) - 1))
  _, stats, tb, _ = _check(sequences, pairs, REALIGNER)
  assert stats.launches == 1 and stats.pairs_on_host == 0
  assert tb.traced_on_device > 250
