"""Seeded batches for the one-launch counting kernel (count_alleles_batch_kernel, csrc/allele_counter.hip;
DV_COUNT_ONE_LAUNCH=1), which maps a workgroup of one grid to (region slot, 64 reads of that region) by bisection of
a block prefix.  The cases put regions on both sides of every step of that mapping:

  block_edge_batch()  read counts 1, 63, 64, 65, 127, 128, 129, 200, 64, 1 -- one workgroup, the last read of one, one
                      more than one, two, three, four -- with a read-less region and a zero-length-interval region
                      between them: neither gets a slot, so region numbers and slot numbers differ from the third
                      region on (results are indexed by region, descriptors by slot);
  special_batch()     between two ordinary regions: one whose first workgroup's reads span more than the 4,096
                      positions of the LDS window and has a read in front of its first read (reference counts go
                      straight to memory on both sides of the window), one whose 64 reads leave more than the 1,024
                      events a workgroup stages in LDS, and one counted with keep_legacy_behavior and higher quality
                      thresholds than its neighbours (each workgroup must read its own region's options);
  `track`             either batch with track_ref_reads and candidate positions on every second batched region, so a
                      region with a candidate mask stands beside one whose mask pointer is null.

Building a case needs no GPU; everything is seeded and built once (functools.lru_cache): tests must not modify what
they get.  tests/test_count_one_launch_cpu.py asserts, from the host alone, that each case holds the workgroup counts
it promises; tests/test_hip_count_one_launch.py runs them on the device."""
import collections
import functools

import numpy as np

from deepvariant_amd import dv_types as T
from tests import batch_edge_cases as E

READS_PER_BLOCK = 64                   # 4 waves x kReadsPerWave
WINDOW = 4096                          # kWindow: positions of a workgroup's LDS window
BLOCK_EVENTS = 1024                    # kBlockEvents: events a workgroup stages in LDS
EDGE_READ_COUNTS = (1, 63, 64, 65, 127, 128, 129, 200, 64, 1)

# spans, reads, options: one per region.  blocks: ceil(n_reads / 64) for a region that gets a slot, else 0.
Case = collections.namedtuple('Case', 'name ref spans reads options blocks total_blocks kinds')
_PLAIN = dict(min_mapping_quality=10, min_base_quality=10, keep_legacy_behavior=False)


class SeqRef:
  def __init__(self, seq):
    self.seq = seq

  def n_bases(self, contig):
    return len(self.seq)

  def get_bases(self, contig, start, end):
    return self.seq[start:end]


def _other(base):
  return 'A' if base != 'A' else 'C'


def _read(ref, name, start, length, rng, substitute=(), insert_at=None, delete_at=None, mapq=60, quals=None):
  """A read of `length` reference positions from `start`: substitutions at the offsets `substitute`, a two-base
  insertion behind offset insert_at, a three-base deletion behind offset delete_at."""
  seq, cigar, run = [], [], 0
  p = start
  while p < start + length:
    off = p - start
    base = ref.seq[p]
    seq.append(_other(base) if off in substitute else base)
    run += 1
    p += 1
    if off == insert_at:
      cigar += [T.CigarUnit(1, run), T.CigarUnit(2, 2)]
      seq += ['G', 'T']
      run = 0
    elif off == delete_at:
      cigar += [T.CigarUnit(1, run), T.CigarUnit(3, 3)]
      p += 3
      run = 0
  if run:
    cigar.append(T.CigarUnit(1, run))
  if quals is None:
    quals = np.full(len(seq), 30, np.uint8)
  return T.Read(fragment_name=name, read_number=1, number_reads=2, aligned_sequence=''.join(seq),
                aligned_quality=bytes(np.asarray(quals, np.uint8)[:len(seq)]),
                alignment=T.LinearAlignment(position=T.Position('c', start, False), mapping_quality=mapq, cigar=cigar))


def _ordinary_reads(ref, rng, name, n, start, end):
  """n reads of 40 to 60 bases over [start - 20, end - 30), position-sorted: every read but each third has a
  substitution, every fifth an insertion, every seventh a deletion; a region's only read has its substitution inside the interval."""
  starts = np.sort(rng.integers(start - 20, end - 30, size=n))
  if n:
    starts[0] = max(starts[0], start)              # so that one read's substitution surely lies in the interval
    starts = np.sort(starts)
  reads = []
  for i, s in enumerate(starts.tolist()):
    length = int(rng.integers(40, 61))
    subs = (int(rng.integers(3, 15)),) if i % 3 != 2 or i == 0 else ()
    reads.append(_read(ref, '%s_%d' % (name, i), s, length, rng, substitute=subs,
                       insert_at=20 if i % 5 == 1 else None, delete_at=25 if i % 7 == 3 else None))
  return reads


def _blocks(n_reads, span):
  return -(-n_reads // READS_PER_BLOCK) if n_reads and span[1] > span[0] else 0


def _finish(name, ref, spans, reads, options, kinds):
  blocks = tuple(_blocks(len(r), s) for r, s in zip(reads, spans))
  return Case(name, ref, tuple(spans), tuple(tuple(r) for r in reads), tuple(options), blocks, sum(blocks), tuple(kinds))


@functools.lru_cache(maxsize=None)
def _reference():
  rng = np.random.default_rng(20261201)
  return SeqRef(''.join('ACGT'[int(i)] for i in rng.integers(0, 4, size=60000)))


@functools.lru_cache(maxsize=None)
def block_edge_batch():
  """Twelve regions: the ten of EDGE_READ_COUNTS, 1 kb each at different contig offsets, with a read-less region
  third and a zero-length-interval region (which has reads) seventh."""
  ref = _reference()
  rng = np.random.default_rng(20261202)
  spans, reads, kinds = [], [], []
  counts = list(EDGE_READ_COUNTS)
  k = 0
  while counts:
    start = 1000 + 2100 * k + 37 * (k % 5)
    if k == 2:
      spans.append((start, start + 1000))
      reads.append([])
      kinds.append('readless')
    elif k == 6:
      spans.append((start + 500, start + 500))
      reads.append(_ordinary_reads(ref, rng, 'z', 70, start, start + 1000))
      kinds.append('zero_length')
    else:
      n = counts.pop(0)
      spans.append((start, start + 1000))
      reads.append(_ordinary_reads(ref, rng, 'r%d' % k, n, start, start + 1000))
      kinds.append('reads%d' % n)
    k += 1
  return _finish('block_edge', ref, spans, reads, [_PLAIN] * len(spans), kinds)


@functools.lru_cache(maxsize=None)
def special_batch():
  ref = _reference()
  rng = np.random.default_rng(20261203)
  spans, reads, options, kinds = [], [], [], []

  def add(kind, span, rs, opts=_PLAIN):
    spans.append(span)
    reads.append(rs)
    options.append(opts)
    kinds.append(kind)

  add('neighbour', (30000, 31000), _ordinary_reads(ref, rng, 'n0', 64, 30000, 31000))
  # a first workgroup (40 reads: one workgroup) that reaches 4,500 positions past its first read, with a last read
  # that starts IN FRONT of the first: reference counts on both sides of the LDS window go straight to memory
  wide = _ordinary_reads(ref, rng, 'w_near', 15, 32000, 32400) + _ordinary_reads(ref, rng, 'w_far', 24, 36500, 37000)
  wide.append(_read(ref, 'w_before', 32000 - 15, 50, rng, substitute=(20,)))
  add('wide', (32000, 37000), wide)
  # 64 reads of 100 bases, every fourth base substituted: 25 events a read, 1,600 in the one workgroup
  noisy = [_read(ref, 'e%d' % i, 40000 + 5 * i, 100, rng, substitute=tuple(range(1, 100, 4))) for i in range(64)]
  add('events', (40000, 40500), noisy)
  # legacy behaviour and higher thresholds: a third of the reads below the mapping quality, base qualities on
  # both sides of 25 (with keep_legacy_behavior a low-quality base leaves nothing; without it, a low-quality allele)
  legacy = []
  starts = np.sort(rng.integers(42000, 42900, size=90)).tolist()
  for i, s in enumerate(starts):
    quals = rng.integers(15, 40, size=64)
    legacy.append(_read(ref, 'l%d' % i, s, int(rng.integers(40, 61)), rng, substitute=(5, 30), insert_at=18 if i % 4 == 0 else None,
                        delete_at=22 if i % 6 == 1 else None, mapq=20 if i % 3 == 0 else 50, quals=quals))
  add('legacy', (42000, 43000), legacy, dict(min_mapping_quality=30, min_base_quality=25, keep_legacy_behavior=True))
  add('neighbour', (44000, 45000), _ordinary_reads(ref, rng, 'n1', 65, 44000, 45000))
  return _finish('special', ref, spans, reads, options, kinds)


def batched_regions(case):
  """The regions that get a slot, in slot order."""
  return [k for k, b in enumerate(case.blocks) if b]


def candidate_positions(case):
  """For the `track` variant: positions on every second batched region (every ninth position of its interval), none
  on the others -- their candidate mask pointer is null."""
  slots = batched_regions(case)
  return [tuple(range(s + 4, e, 9)) if k in slots and slots.index(k) % 2 == 0 else () for k, (s, e) in enumerate(case.spans)]


def counters(case, track=False, only=None):
  """Fresh AlleleCounters, one per region (`only`: that region alone)."""
  from deepvariant_amd import allelecounter as A
  positions = candidate_positions(case) if track else [()] * len(case.spans)
  out = []
  for k, ((s, e), rs, opts) in enumerate(zip(case.spans, case.reads, case.options)):
    if only is not None and k != only:
      continue
    c = A.AlleleCounter(case.ref, 'c', s, e, candidate_positions=positions[k], track_ref_reads=track, **opts)
    for r in rs:
      c.add(r)
    out.append(c)
  return out


# the regions past 256 slots are batch_edge_cases': (slots with reads, the slot that overflows or None)
MANY_REGIONS = ((257, None), (300, None), (300, 260))


def many_regions(n, overflow_at=None):
  return E.edge_regions(n, overflow_at)
