"""dv_local_align_pairs_device (csrc/local_align.hip: both Smith-Waterman sweeps of every pair in one
kernel launch, CIGARs on the host) against dv_local_align, the scalar host aligner that the libssw
vectors pin: pair by pair, every field including the CIGAR text.

The kernel gives lane l of a wave the query rows [l*S, (l+1)*S), S = ceil(|q| / 64) rounded up to
one of the buckets 1 2 3 4 8 16 24 32, so the query lengths below sit on both sides of every
multiple of 64 up to 192 and of every bucket edge (256, 512, 1024, 1536, 2048 = the device limit).
"""
import numpy as np
import pytest

from deepvariant_amd import _lib
from deepvariant_amd import fast_pass_aligner as F

pytestmark = pytest.mark.gpu

LETTERS = np.array(list('ACGT'))
DEFAULT = (2, 2, 3, 1)
REALIGNER = (4, 6, 8, 1)


def _fields(a):
  return (a.score, a.ref_begin, a.ref_end, a.query_begin, a.query_end, a.mismatches, bytes(a.cigar))


def _host(reference, query, scoring):
  """dv_local_align, or None where it refuses (an empty sequence)."""
  try:
    return _fields(F.local_align(reference, query, *scoring))
  except _lib.DvError:
    return None


def _check(sequences, pairs, scoring, on_host=0):
  """One device call over `pairs`; every result against the host aligner.  -> (results, stats)"""
  got, stats = F.local_align_pairs_device(sequences, pairs, scoring, with_stats=True)
  assert len(got) == len(pairs)
  for (r, q), g in zip(pairs, got):
    want = _host(sequences[r], sequences[q], scoring)
    assert (None if g is None else _fields(g)) == want, (len(sequences[r]), len(sequences[q]), scoring,
                                                        sequences[r][:80], sequences[q][:80])
  device_pairs = [(r, q) for r, q in pairs if sequences[r] and sequences[q]]
  assert stats.pairs == len(pairs) and stats.pairs_on_host == on_host
  assert stats.launches == (1 if len(device_pairs) > on_host else 0)
  return got, stats


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


def test_libssw_vectors():
  """The vectors of tests/test_fast_pass_aligner_cpu.py (ssw_wrap_test.cc, ssw_test.cc), both ways round."""
  ref, query = 'CAGCCTTTCTGACCCGGAAATCAAAATAGGCACAACAAA', 'CTGAGCCGGTAAATC'
  got, _ = _check([ref, query], [(0, 1), (1, 0)], DEFAULT)
  assert _fields(got[0]) == (21, 8, 21, 0, 14, 2, b'4=1X4=1I5=')
  assert _fields(got[1])[:1] + _fields(got[1])[6:] == (21, b'8S4=1X4=1D5=17S')
  got, _ = _check(['tttt', 'ttAtt', 'TTTTGGGGGGGGGGGGG', 'TTATTGGGGGGGGGGGGG'], [(0, 1), (2, 3)], (4, 2, 4, 2))
  assert [bytes(g.cigar) for g in got] == [b'2=1I2=', b'2=1I15=']
  got, _ = _check(['TTTGCCGAAGTTAAACCC', 'GCCGAAGTTA'], [(0, 1)], REALIGNER)
  assert bytes(got[0].cigar) == b'10=' and got[0].ref_begin == 3


@pytest.mark.parametrize('seed,scoring', [(1, (4, 6, 8, 2)), (2, (2, 2, 3, 1)), (3, (1, 4, 6, 1)), (4, (4, 6, 8, 1))])
def test_mutated_pieces_junk_repeats_and_n_runs(seed, scoring):
  """The generator of test_batched_alignment_equals_one_at_a_time, same seeds and scorings."""
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
  _check(sequences, [(0, k) for k in range(1, len(sequences))], scoring)
  _check(sequences, [(0, 1)], scoring)                                     # and a batch of one


QUERY_LENGTHS = [1, 2, 63, 64, 65, 127, 128, 129, 150, 191, 192, 193, 255, 256, 257, 511, 512, 513,
                 1023, 1024, 1025, 1535, 1536, 1537, 2047, 2048, 2049]
REFERENCE_LENGTHS = [1, 2, 64, 65, 300, 1400]


@pytest.mark.parametrize('scoring', [REALIGNER, DEFAULT])
def test_every_kernel_boundary(scoring):
  """Query lengths around every multiple of 64 up to 192, every rows-per-lane bucket edge, the device limit
  and limit + 1 (which must go to the host code and still match), against reference lengths 1 .. 1,400:
  shorter than, equal to and longer than the query.  The query holds a lightly edited copy of (a piece
  of) the reference at its start, middle or end, so end points fall into first, inner and last lanes."""
  assert QUERY_LENGTHS[-2] == _lib.DV_LOCAL_ALIGN_DEVICE_MAX_QUERY
  rng = np.random.default_rng(11)
  sequences, pairs = [], []
  references = [_random(rng, m) for m in REFERENCE_LENGTHS]
  sequences += references
  for n in QUERY_LENGTHS:
    for r, reference in enumerate(references):
      take = min(n, len(reference))
      a = int(rng.integers(0, len(reference) - take + 1))
      core = _mutated(rng, reference[a:a + take], int(rng.integers(0, 4)))[:n]
      where = (len(pairs) % 3) * (n - len(core)) // 2
      query = _random(rng, where) + core + _random(rng, n - len(core) - where)
      assert len(query) == n
      pairs.append((r, len(sequences)))
      sequences.append(query)
  _, stats = _check(sequences, pairs, scoring, on_host=len(REFERENCE_LENGTHS))
  assert stats.cells == sum(len(sequences[r]) * len(sequences[q]) for r, q in pairs
                            if len(sequences[q]) <= _lib.DV_LOCAL_ALIGN_DEVICE_MAX_QUERY)


def test_reference_past_the_device_limit_goes_to_the_host():
  rng = np.random.default_rng(5)
  long_ref = _random(rng, _lib.DV_LOCAL_ALIGN_DEVICE_MAX_REFERENCE + 1)
  at_limit = long_ref[:-1]
  query = _mutated(rng, long_ref[65_000:65_150], 2)
  _check([long_ref, at_limit, query], [(0, 2), (1, 2)], REALIGNER, on_host=1)


def test_ties_go_to_the_first_column_and_the_smallest_row():
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
    _check(sequences, pairs, scoring)


def test_degenerate_inputs():
  sequences = ['ACGTACGTAC', 'NNNNNNN', 'AAAAAAAA', 'CCCCC', '', 'N', 'ACNNGT', 'ACNNGTACNNGTAC']
  pairs = [(0, 1), (1, 0), (1, 1), (2, 3), (3, 2), (0, 4), (4, 0), (4, 4), (5, 5), (6, 7), (7, 6), (6, 6)]
  got, _ = _check(sequences, pairs, DEFAULT)
  assert got[0].score == 0 and bytes(got[0].cigar) == b''        # an all-N query: nothing aligns, no CIGAR
  assert got[2].score == 0 and got[3].score == 0                 # N does not match N; no common base
  assert got[5] is None and got[6] is None and got[7] is None    # empty sequences: score -1
  _check(sequences, pairs, REALIGNER)


def test_scores_past_the_int16_range_of_the_host_lanes():
  rng = np.random.default_rng(13)
  reference = _random(rng, 900)
  queries = [_mutated(rng, reference[200:600], 3)[:400], reference[100:500], reference[300:500] + 'N' + reference[501:700]]
  got, _ = _check([reference] + queries, [(0, 1), (0, 2), (0, 3)], (100, 6, 8, 1))
  assert got[1].score == 100 * 400 > 32767


@pytest.mark.parametrize('n_pairs', [1, 3, 300])
def test_batch_sizes(n_pairs):
  rng = np.random.default_rng(100 + n_pairs)
  references = [_random(rng, int(rng.integers(200, 500))) for _ in range(min(n_pairs, 7))]
  sequences, pairs = list(references), []
  for k in range(n_pairs):
    r = k % len(references)
    a = int(rng.integers(0, len(references[r]) - 150))
    sequences.append(_mutated(rng, references[r][a:a + int(rng.integers(30, 151))], int(rng.integers(0, 5))))
    pairs.append((r, len(sequences) - 1))
  _check(sequences, pairs, REALIGNER)


def test_one_haplotype_shared_by_fifty_reads():
  rng = np.random.default_rng(17)
  haplotype = _random(rng, 600)
  reads = [_mutated(rng, haplotype[a:a + 150], int(rng.integers(0, 4)))
           for a in rng.integers(0, 450, size=50).tolist()]
  _, stats = _check([haplotype] + reads, [(0, k + 1) for k in range(50)], REALIGNER)
  assert stats.cells == sum(600 * len(r) for r in reads)
