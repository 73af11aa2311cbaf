"""Shared cases for the window-trimming tests (test_trim_reads_cpu.py, test_hip_trim_reads.py): reads with chosen
CIGARs and the windows that cut them, the reference arrays from alt_aligned_pileup_lib.trim_reads on Read objects
(the checker), and a transcription of the closed form that csrc/trim_reads.hip states and its kernels compute.

A case is (name, reads, windows); a window is (q0, q1, r0, r1, min_overlap) -- the read query, the pileup
window, the least reference overlap.  Everything is built once and shared (functools.lru_cache); tests must
not modify what they get."""
import collections
import functools

import numpy as np

from deepvariant_amd import alt_aligned_pileup_lib as A
from deepvariant_amd import dv_types as T
from deepvariant_amd import packing

Case = collections.namedtuple('Case', 'name reads windows')

M, I, D, N, S, H, P, EQ, X = 1, 2, 3, 4, 5, 6, 7, 8, 9
REF_OPS = (M, D, N, EQ, X)
READ_OPS = (M, I, S, EQ, X)
ARRAYS = ('window_row_off', 'src_row', 'pos', 'end', 'read_trim', 'new_len', 'cigar_off', 'cigar')
CONTIG = 20000
WIDTH = 61


def make_read(name, pos, ops, rng, short_by=0, number=0):
  """A Read with the CIGAR `ops` [(operation, length), ...]; `short_by` bases fewer than the CIGAR consumes."""
  qlen = sum(ln for op, ln in ops if op in READ_OPS) - short_by
  return T.Read(
      fragment_name=name, read_number=number, number_reads=2, fragment_length=int(rng.integers(-900, 900)),
      aligned_sequence=''.join('ACGT'[int(j)] for j in rng.integers(0, 4, size=qlen)),
      aligned_quality=bytes(rng.integers(0, 60, size=qlen).astype(np.uint8)),
      alignment=T.LinearAlignment(position=T.Position('chr1', int(pos), bool(rng.integers(0, 2))),
                                  mapping_quality=int(rng.integers(1, 60)),
                                  cigar=[T.CigarUnit(op, ln) for op, ln in ops]))


def _ref_prefix(ops):
  r = [0]
  for op, ln in ops:
    r.append(r[-1] + (ln if op in REF_OPS else 0))
  return r


def _window(r0, r1, min_overlap=A.K_DEFAULT_MINIMUM_READ_OVERLAP, q=None):
  """A window whose query is the window itself unless `q` says otherwise (the C entry points take both)."""
  q0, q1 = q if q is not None else (r0, r1)
  return (int(q0), int(q1), int(r0), int(r1), int(min_overlap))


def _long_ops(n):
  """n operations: a leading S, then M I M D M N ... so every kind sits on both sides of the 64-lane chunk ends."""
  cycle = [(M, 5), (I, 2), (M, 4), (D, 3), (EQ, 6), (N, 7), (X, 3), (I, 1), (M, 2), (P, 1), (D, 1), (M, 8)]
  ops = [(S, 4)] + [cycle[k % len(cycle)] for k in range(n - 1)]
  return ops[:n]


def _chunk_case(n_ops, rng):
  """One read of n_ops operations and windows that start / end at, just inside and just behind the operations
  around indices 0, 63, 64, 65, 128 (where they exist), so a and b fall on both sides of the chunk boundaries."""
  pos = 5000
  ops = _long_ops(n_ops) if n_ops > 1 else [(M, 100)]
  reads = [make_read('long%d' % n_ops, pos, ops, rng),
           make_read('mate%d' % n_ops, pos + 7, [(M, 60)], rng, number=1)]     # shares every window near the start
  R = _ref_prefix(ops)
  marks = sorted({k for k in (0, 1, 2, 61, 62, 63, 64, 65, 66, 126, 127, 128, 129) if k < n_ops})
  windows = [_window(pos - 50, pos + R[-1] + 50), _window(pos - 50, pos + R[-1] + 50, WIDTH)]   # the whole read
  for k in marks:
    for r0 in {pos + R[k], pos + R[k] + 1, pos + R[k + 1] - 1} if R[k + 1] > R[k] else {pos + R[k]}:
      windows.append(_window(r0, r0 + WIDTH))                       # starts at / inside operation k
      windows.append(_window(r0, pos + R[-1] + 10))                 # ... and runs to the read's end
    for r1 in {pos + R[k + 1], pos + R[k + 1] - 1, pos + R[k + 1] + 1}:
      if r1 > pos:
        windows.append(_window(pos - 10, r1))                       # ends at / inside / just behind operation k
        if r1 - WIDTH > pos:
          windows.append(_window(r1 - WIDTH, r1, WIDTH))            # a and b both deep in the CIGAR, spanning reads only
  return Case('ops%d' % n_ops, reads, windows)


def _hand_case(rng):
  reads = [
      make_read('plain', 1000, [(M, 50)], rng),                                   # 0: [1000, 1050)
      make_read('ins_at_cut', 1000, [(M, 20), (I, 3), (M, 20)], rng),             # 1: an I on the boundary 1020
      make_read('del', 1000, [(M, 20), (D, 10), (M, 20)], rng),                   # 2: D over [1020, 1030)
      make_read('skip', 1000, [(M, 20), (N, 30), (M, 20)], rng),                  # 3: N over [1020, 1050)
      make_read('clip', 1000, [(S, 5), (M, 30), (S, 4)], rng),                    # 4: soft clips at both ends
      make_read('tail_only', 960, [(M, 40), (I, 5), (S, 5)], rng),                # 5: behind 1000 only I / S
      make_read('at_zero', 0, [(M, 45)], rng),                                    # 6
      make_read('near_zero', 3, [(S, 2), (M, 40)], rng),                          # 7
      make_read('at_end', CONTIG - 45, [(M, 45)], rng),                           # 8: ends at the contig's end
      make_read('ins_first', 1000, [(I, 4), (M, 40)], rng),                       # 9: leading I
      make_read('zero_len', 1000, [(M, 20), (M, 0), (D, 0), (I, 2), (M, 20)], rng),   # 10: zero-length operations
  ]
  w = _window
  windows = [
      w(900, 1100),                      # before and behind everything at 1000: whole reads
      w(1000, 1061), w(1000, 1061, WIDTH),
      w(1020, 1081),                     # starts at an operation boundary, the one the I sits on
      w(1010, 1071),                     # inside M
      w(1025, 1086),                     # inside D (read 2) and inside N (read 3)
      w(1049, 1110),                     # last base of N
      w(990, 1020),                      # ends at a boundary followed by I then M: the I stays, then a 0M
      w(990, 1025),                      # ends inside D
      w(990, 1021),
      w(1036, 1100), w(1035, 1100),      # overlap 14 / 15 with 'plain' from the right
      w(900, 1014), w(900, 1015),        # ... from the left
      w(1000, 1100, q=(990, 1100)),      # 'tail_only' joins: only I / S behind 1000 (dropped, span 0)
      w(0, 31), w(0, 41, WIDTH),         # clipped to r0 = 0
      w(CONTIG - 31, CONTIG), w(CONTIG - 61, CONTIG, WIDTH),   # clipped to the contig's end
      w(7000, 7061),                     # no reads
      w(1005, 1030), w(1004, 1031),      # inside the leading clip's M
  ]
  return Case('hand', reads, windows)


def _unsorted_case(rng):
  base = _hand_case(rng)
  order = rng.permutation(len(base.reads))
  return Case('unsorted', [base.reads[int(k)] for k in order], base.windows)


def _random_case(rng, n_reads=300, max_ops=200, n_windows=40, buffer_bp=5):
  from tests import fuzz_inputs as F
  reads = []
  for k in range(n_reads):
    ops = [(int(u.operation), int(u.operation_length)) for u in F.random_cigar(rng, 1, max_ops)]
    ops = [(op, 0 if rng.random() < 0.02 else ln) for op, ln in ops]
    if not any(ln for op, ln in ops if op in READ_OPS):
      ops.append((M, 1))
    reads.append(make_read('r%d' % int(rng.integers(0, n_reads // 2)), int(rng.integers(1000, 4000)), ops, rng,
                           number=int(rng.integers(0, 2))))
  reads.sort(key=lambda r: r.alignment.position.position)
  windows = []
  for _ in range(n_windows):
    width = 2 * int(rng.integers(30, 111)) + 1                       # 61 .. 221
    hw = (width - 1) // 2
    v = int(rng.integers(1000, 5000))
    spanning = rng.random() < 0.25
    windows.append((v - buffer_bp, v + 1 + buffer_bp, max(v - hw, 0), min(CONTIG, v + 1 + hw),
                    width if spanning else A.K_DEFAULT_MINIMUM_READ_OVERLAP))
  return Case('random', reads, windows)


@functools.lru_cache(maxsize=None)
def cases():
  rng = np.random.default_rng(20261019)
  return tuple([_hand_case(rng), _unsorted_case(rng)] + [_chunk_case(n, rng) for n in (1, 63, 64, 65, 130)] +
               [_random_case(rng)])


def case(name):
  return next(c for c in cases() if c.name == name)


CASE_NAMES = ('hand', 'unsorted', 'ops1', 'ops63', 'ops64', 'ops65', 'ops130', 'random')


@functools.lru_cache(maxsize=None)
def table(name):
  return packing.ReadTable.from_reads(case(name).reads)


def _words(cigar):
  return [(int(u.operation_length) << 4) | int(u.operation) for u in cigar]


def _finish(rows, words, offsets, win_off):
  cols = list(zip(*rows)) if rows else [[]] * 5
  out = {name: np.array(cols[k], np.int32) for k, name in enumerate(('src_row', 'pos', 'end', 'read_trim', 'new_len'))}
  out['window_row_off'] = np.array(win_off, np.int32)
  out['cigar_off'] = np.array(offsets, np.uint32)
  out['cigar'] = np.array(words, np.uint32)
  return out


@functools.lru_cache(maxsize=None)
def reference(name):
  """-> (arrays in dv_trimmed_reads_view's layout, the trimmed Read objects, their untrimmed starts), from
  alt_aligned_pileup_lib.trim_reads window by window; read_trim, which trim_reads does not return, from trim_cigar."""
  c = case(name)
  t = table(name)
  rows, words, offsets, win_off = [], [], [0], [0]
  objects, starts = [], []
  for q0, q1, r0, r1, min_overlap in c.windows:
    idx = [int(k) for k in t.query(q0, q1)]
    kept, original = A.trim_reads([c.reads[k] for k in idx], r0, r1, min_overlap)
    it = iter(kept)
    n_kept = 0
    for k in idx:
      read = c.reads[k]
      pos = read.alignment.position.position
      cigar, read_trim, new_len = A.trim_cigar(read.alignment.cigar, max(r0 - pos, 0), r1 - max(r0, pos))
      if A.calculate_cigar_length(cigar) >= min_overlap and new_len > 0:
        got = next(it)
        assert got.alignment.cigar == cigar and len(got.aligned_sequence) == new_len
        new_pos = got.alignment.position.position
        rows.append((k, new_pos, new_pos + A.calculate_cigar_length(cigar), read_trim, new_len))
        words.extend(_words(cigar))
        offsets.append(len(words))
        n_kept += 1
    assert n_kept == len(kept)
    objects.extend(kept)
    starts.extend(original)
    win_off.append(len(rows))
  return _finish(rows, words, offsets, win_off), objects, starts


def closed_form_pair(words, pos, seq_len, r0, r1, min_overlap):
  """The closed form at the top of csrc/trim_reads.hip for one pair, with prefix sums instead of a walk.
  -> None (not kept) or (new pos, end, read_trim, new_len, trimmed words); ValueError where the reference checks."""
  w = np.asarray(words, np.int64)
  n = len(w)
  op, ln = w & 15, w >> 4
  on_ref = np.isin(op, REF_OPS)
  on_read = np.isin(op, READ_OPS)
  R = np.concatenate([[0], np.cumsum(np.where(on_ref, ln, 0))])
  Q = np.concatenate([[0], np.cumsum(np.where(on_read, ln, 0))])
  Tt = max(r0 - pos, 0)
  Cc = r1 - max(r0, pos)
  if Cc <= 0:
    raise ValueError('Check failed: ref_length > 0')
  out = ln.copy()
  if Tt == 0:
    first = np.arange(n)[:1]
  else:
    first = np.nonzero((R[1:] > Tt) | (R[:-1] == Tt))[0][:1]
  if not len(first):
    a, read_trim, last = n, int(Q[n]), n - 1
  else:
    a = int(first[0])
    read_trim = int(Q[a])
    if R[a] < Tt:
      out[a] = R[a + 1] - Tt
      read_trim += int(Tt - R[a]) if on_read[a] else 0
    over = np.nonzero(R[a + 1:] - Tt > Cc)[0][:1]
    if len(over):
      last = a + int(over[0])
      out[last] = Cc - (max(int(R[last]), Tt) - Tt)
    else:
      last = n - 1
  kept = slice(a, last + 1)
  new_len = int(out[kept][on_read[kept]].sum())
  span = int(out[kept][on_ref[kept]].sum())
  if read_trim + new_len > seq_len:
    raise ValueError('Check failed: read_trim + new_read_length <= aligned_sequence.size()')
  if span < min_overlap or new_len <= 0:
    return None
  new_pos = r0 if Tt != 0 else pos
  return new_pos, new_pos + span, read_trim, new_len, ((out[kept] << 4) | op[kept]).tolist()


def closed_form(name):
  """closed_form_pair over a case's table, in the layout of `reference`."""
  c = case(name)
  t = table(name)
  rows, words, offsets, win_off = [], [], [0], [0]
  seq_len = np.diff(t.read_seq_off.astype(np.int64))
  for q0, q1, r0, r1, min_overlap in c.windows:
    for k in t.query(q0, q1).tolist():
      got = closed_form_pair(t.cigar[t.read_cigar_off[k]:t.read_cigar_off[k + 1]], int(t.read_pos[k]),
                             int(seq_len[k]), r0, r1, min_overlap)
      if got is not None:
        rows.append((k,) + got[:4])
        words.extend(got[4])
        offsets.append(len(words))
    win_off.append(len(rows))
  return _finish(rows, words, offsets, win_off)


def assert_same_arrays(got, want, what):
  for name in ARRAYS:
    assert got[name].dtype == want[name].dtype, (what, name)
    np.testing.assert_array_equal(got[name], want[name], err_msg='%s: %s' % (what, name))


# ---- the two inputs the reference refuses
def cover_error_case():
  """C <= 0: a read query wider than the pileup window's half width reaches a read that starts behind the window."""
  rng = np.random.default_rng(5)
  reads = [make_read('inside', 1000, [(M, 80)], rng), make_read('behind', 1090, [(M, 50)], rng)]
  v = 1040
  return Case('cover', reads, [_window(v - 30, v + 31, q=(v - 100, v + 101))])


def length_error_case():
  """A CIGAR that consumes more bases than the read has (ReadTable.from_reads refuses to pack one, so the table is
  that of the whole read with the last 10 bases taken away again)."""
  import dataclasses
  rng = np.random.default_rng(6)
  whole = [make_read('fine', 1000, [(M, 60)], rng), make_read('short', 1000, [(M, 60)], rng)]
  t = packing.ReadTable.from_reads(whole)
  seq_off = t.read_seq_off.copy()
  seq_off[-1] -= 10
  t = dataclasses.replace(t, read_seq_off=seq_off, bases=t.bases[:-10].copy(), quals=t.quals[:-10].copy())
  short = dataclasses.replace(whole[1], aligned_sequence=whole[1].aligned_sequence[:-10],
                              aligned_quality=whole[1].aligned_quality[:-10])
  return Case('length', [whole[0], short], [_window(990, 1100)]), t
