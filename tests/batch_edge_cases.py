"""Seeded batches that put a chosen element on the far side of the step of the five loops that turn per-element
counts into output offsets and carry a running total from step to step:

  alt_finish_scan_kernel (csrc/alt_align.hip), pack_scan_kernel (csrc/pack_regions.hip) and trim_scan_kernel
  (csrc/trim_reads.hip) step 1,024 elements at a time: pairs, candidates, pairs;
  cand_pack_kernel (csrc/candidates.hip) and gvcf_pack_kernel (csrc/gvcf.hip) sum 256 regions per step.

Every builder takes the wanted count and returns a case with exactly that many elements, built on the case modules
of the kernels' own tests (alt_align_cases, pack_cases, trim_cases, the helpers of test_hip_candidates.py and
test_hip_gvcf.py).  Elements are as small as the kernels allow, so that the host checkers cost milliseconds.
Building a case needs no GPU; everything is seeded and built once (functools.lru_cache): tests must not modify
what they get.  tests/test_batch_edges_cpu.py asserts, from the host's answers alone, that each case holds what it
promises here; tests/test_hip_batch_edges.py runs them on the device."""
import collections
import functools

import numpy as np

from deepvariant_amd import packing
from tests import alt_align_cases as AC
from tests import pack_cases as PC
from tests import trim_cases as TC

SCAN_STEP = 1024                       # kScanThreads of the three scan kernels
SCAN_SIZES = (1023, 1024, 1025, 2048, 2049)
REGION_STEP = 256                      # kThreads of the two pack kernels
REGION_SIZES = (257, 300)              # regions with reads: the workgroups of the pack kernels


# ---------------------------------------------------------------- alt-align: pairs
_ALT_READS = 96
_ALT_SEED = 20261103                   # with it pairs 1,023, 1,024, 2,047 and 2,048 all write words (asserted on the CPU)


@functools.lru_cache(maxsize=None)
def _alt_align_stream():
  """The reads, the targets and an item stream of SCAN_SIZES[-1] pairs that every size is a prefix of, so pair k is
  the same pair in every case that holds it.  96 reads of 8 to 60 bases drawn with alt_align_cases._edited from
  five targets of about 80 bytes (the second an indel variant of the first), every sixth read poly-A (status 2),
  then the four reads of the `kinds` batch's items 1 and 2 with their targets; those two items stand at the
  stream's start and again behind pair 1,100, so that the pair `unnormalised` (status 0 without normalize_reads)
  lies on both sides of the step."""
  rng = np.random.default_rng(_ALT_SEED)
  base = AC._seq(rng, 80)                                                     # pylint: disable=protected-access
  targets = [base, base[:40] + 'GT' + base[43:], AC._seq(rng, 78), AC._seq(rng, 82), AC._seq(rng, 80)]   # pylint: disable=protected-access
  seqs = []
  for k in range(_ALT_READS):
    if k % 6 == 5:
      seqs.append('A' * int(rng.integers(8, 61)))
    else:
      seqs.append(AC._edited(rng, targets[k % len(targets)])[:60])           # pylint: disable=protected-access
  reads, starts = AC._reads(rng, seqs, 'e')                                   # pylint: disable=protected-access
  kinds = AC.kinds_batch()
  first, n_main = kinds['items'][1][0], kinds['items'][0][1]
  assert first == n_main and kinds['items'][2][0] == first + 2
  reads = reads + kinds['reads'][first:first + 4]
  starts = starts + kinds['starts'][first:first + 4]
  targets = targets + kinds['targets'][1:3]
  kind_items = [(_ALT_READS, 2, 5, AC.REF_START, kinds['items'][1][4]),
                (_ALT_READS + 2, 2, 6, AC.REF_START + 500, kinds['items'][2][4])]
  items, total, again = list(kind_items), 4, False
  while total < SCAN_SIZES[-1]:
    if total > 1100 and not again:
      items += kind_items
      total += 4
      again = True
      continue
    n_rows = int(rng.integers(1, _ALT_READS + 1))
    first_row = int(rng.integers(0, _ALT_READS - n_rows + 1))
    items.append((first_row, n_rows, int(rng.integers(0, 5)), AC.REF_START + int(rng.integers(0, 20)),
                  AC.read_size_of(seqs[first_row:first_row + n_rows])))
    total += n_rows
  return reads, starts, targets, items


@functools.lru_cache(maxsize=None)
def edge_alt_align(n_pairs):
  """-> a batch in alt_align_cases' form with exactly n_pairs pairs: the stream's items, the last one cut to fit."""
  reads, starts, targets, stream = _alt_align_stream()
  items, total = [], 0
  for first_row, n_rows, target, ref_start, read_size in stream:
    if total == n_pairs:
      break
    n_rows = min(n_rows, n_pairs - total)
    items.append((first_row, n_rows, target, ref_start, read_size))
    total += n_rows
  assert total == n_pairs
  return dict(name='edge%d' % n_pairs, reads=reads, starts=starts, items=items, targets=targets, cfg=dict(AC.CFG),
              kinds={})


@functools.lru_cache(maxsize=None)
def alt_align_table(n_pairs):
  return AC.table_of(edge_alt_align(n_pairs))


# ---------------------------------------------------------------- trim: pairs
_TRIM_READS, _TRIM_POS, _TRIM_STEP = 64, 1000, 3
_TRIM_SHAPES = ([(TC.M, 40)],
                [(TC.S, 3), (TC.M, 20), (TC.I, 2), (TC.M, 20)],
                [(TC.M, 20), (TC.D, 4), (TC.M, 20)],
                [(TC.M, 10), (TC.I, 1), (TC.M, 15), (TC.D, 2), (TC.M, 15), (TC.S, 4)])
# where a window is cut so that the next window's first pair is pair 1,024 (2,048)
_TRIM_CUTS = {1025: (SCAN_STEP,), 2049: (SCAN_STEP, 2 * SCAN_STEP)}
# one window walk per size.  With these seeds pairs 1,023 and 1,024 are (kept, kept) for 1,025 and 2,049 pairs and
# (kept, not kept) for 2,048; pairs 2,047 and 2,048 of the 2,049-pair case are both kept (asserted on the CPU)
_TRIM_SEEDS = {1023: 1, 1024: 2, 1025: 3, 2048: 21, 2049: 8}


@functools.lru_cache(maxsize=None)
def _trim_reads():
  rng = np.random.default_rng(20261102)
  reads = [TC.make_read('t%d' % (k // 2), _TRIM_POS + _TRIM_STEP * k, _TRIM_SHAPES[k % 4], rng, number=k % 2)
           for k in range(_TRIM_READS)]
  return reads, packing.ReadTable.from_reads(reads)


def _narrowed(table, window, want):
  """`window` with its query narrowed from the right until it names exactly `want` reads; where no such query
  exists, a window over the first reads (they start 3 bases apart, so every count up to 21 has a query)."""
  q0, q1, r0, r1, min_overlap = window
  for end in range(q1, q0, -1):
    if len(table.query(q0, end)) == want:
      return (q0, end, r0, r1, min_overlap)
  head = (_TRIM_POS - 10, _TRIM_POS + _TRIM_STEP * (want - 1) + 1, _TRIM_POS - 10, _TRIM_POS + 61, 15)
  assert len(table.query(head[0], head[1])) == want, want
  return head


@functools.lru_cache(maxsize=None)
def edge_trim(n_pairs):
  """-> trim_cases.Case with exactly n_pairs (window, read) pairs: 64 reads 3 bases apart in four short CIGAR
  shapes, windows of 31 to 71 bases walking over them with min_overlap 15 or the full width.  A window that would
  pass a cut (the total, and for 1,025 and 2,049 pairs also 1,024 and 2,048) has its query narrowed to end on it."""
  reads, table = _trim_reads()
  rng = np.random.default_rng(_TRIM_SEEDS[n_pairs])
  cuts = list(_TRIM_CUTS.get(n_pairs, ())) + [n_pairs]
  windows, total, at = [], 0, _TRIM_POS - 20
  last = _TRIM_POS + _TRIM_STEP * _TRIM_READS
  while total < n_pairs:
    width = int(rng.integers(31, 72))
    window = (at, at + width, at, at + width, width if rng.random() < 0.4 else 15)
    at += int(rng.integers(1, 12))
    if at > last:
      at = _TRIM_POS - 20
    count = len(table.query(window[0], window[1]))
    cut = next(c for c in cuts if c > total)
    if total + count > cut:
      window = _narrowed(table, window, cut - total)
      count = cut - total
    windows.append(window)
    total += count
  return TC.Case('edge%d' % n_pairs, reads, windows)


def trim_table(n_pairs):
  """The packed table of a case's reads (every size shares the 64 reads)."""
  return _trim_reads()[1]


def trim_closed_form(case, table):
  """trim_cases.closed_form over any case -> (arrays in the layout of trim_cases.reference, kept flag per pair,
  first pair of every window and the total)."""
  rows, words, offsets, win_off, kept, pair_off = [], [], [0], [0], [], [0]
  seq_len = np.diff(table.read_seq_off.astype(np.int64))
  for q0, q1, r0, r1, min_overlap in case.windows:
    for k in table.query(q0, q1).tolist():
      got = TC.closed_form_pair(table.cigar[table.read_cigar_off[k]:table.read_cigar_off[k + 1]], int(table.read_pos[k]),
                                int(seq_len[k]), r0, r1, min_overlap)
      kept.append(got is not None)
      if got is not None:
        rows.append((k,) + got[:4])
        words.extend(got[4])
        offsets.append(len(words))
    win_off.append(len(rows))
    pair_off.append(len(kept))
  return TC._finish(rows, words, offsets, win_off), np.array(kept, bool), pair_off    # pylint: disable=protected-access


@functools.lru_cache(maxsize=None)
def trim_expected(n_pairs):
  return trim_closed_form(edge_trim(n_pairs), trim_table(n_pairs))


# ---------------------------------------------------------------- pack: candidates
WIDE_COMBOS = (257, 513)


def _small_region(seed, name, n_cands, shuffle, forced=None):
  """About 200 reads under 90 fragment names, n_cands candidates sorted by position with 0 to 3 combination masks,
  about one in eleven without a reference window, short support lists with a ghost key.  Sorted regions get a long
  first read, as pack_cases.generator_region's.  `forced`: {candidate index: has a reference window}; a forced
  candidate has at least one mask."""
  rng = np.random.default_rng(seed)
  n = 200
  pos = rng.integers(0, 900, size=n)
  span = rng.integers(1, 100, size=n)
  names = ['%s%d' % (name, int(x)) for x in rng.integers(0, 90, size=n)]
  number = rng.integers(0, 2, size=n)
  if not shuffle:
    order = np.argsort(pos, kind='stable')
    pos, span, number = pos[order], span[order], number[order]
    names = [names[i] for i in order]
    pos[0], span[0] = 0, 950
  region = PC.Region(name, pos, pos + span, names, number, [])
  keys = region.keys
  forced = forced or {}
  for k, p in enumerate(sorted(rng.integers(20, 880, size=n_cands).tolist())):
    n_alts = int(rng.integers(1, 4))
    n_masks = int(rng.integers(0, 4))
    window = k % 11 != 7
    if k in forced:
      window, n_masks = forced[k], max(n_masks, 1)
    cand = PC.Candidate(p, p + 1, n_alts, PC._all_masks(n_alts)[:n_masks], [], window=window)   # pylint: disable=protected-access
    near = region.picked(cand)
    support = [(PC.GHOST, int(rng.integers(0, n_alts)))]
    for alt in range(n_alts):
      rows = list(rng.choice(near, size=min(len(near), int(rng.integers(0, 4))), replace=False)) if len(near) else []
      rows += rng.integers(0, n, size=int(rng.integers(0, 2))).tolist()
      support += [(keys[int(r)], alt) for r in rows]
    if n_alts >= 2 and len(near):
      r = int(near[int(rng.integers(0, len(near)))])
      support += [(keys[r], n_alts - 1), (keys[r], 0)]                # the larger alt first in list order
    order = rng.permutation(len(support))
    cand.support = [support[int(i)] for i in order]
    region.candidates.append(cand)
  return region


def wide_region():
  """A 65-read pile with two candidates of 32 alts that carry 257 and 513 random non-zero combination masks: the
  `k += kThreads` item loop of pack_emit_kernel takes a second and a third step."""
  rng = np.random.default_rng(20261104)
  n = 65
  pos = np.full(n, 7000)
  names = ['w%d' % i for i in range(n)]
  cands = []
  for k, n_masks in enumerate(WIDE_COMBOS):
    masks = rng.integers(1, 1 << 32, size=n_masks, dtype=np.uint64).tolist()
    support = [('w%d/0' % i, int(rng.integers(0, 32))) for i in range(0, n, 2)] + [('w7/0', 0), ('w8/0', 31), (PC.GHOST, 3)]
    cands.append(PC.Candidate(7050 + k, 7051 + k, 32, masks, support))
  return PC.Region('wide', pos, pos + 100, names, np.zeros(n, np.uint8), cands)


PackCase = collections.namedtuple('PackCase', 'regions edge')
# per size: the regions as (kind, candidates), and what candidates 1,023 and 1,024 are.
#   'inside': both in one region, both give items; 'first': 1,024 is its region's first candidate; 'skipped':
#   1,023 has no reference window (the element that makes the carry adds nothing) between two that give items
_PACK_LAYOUT = {
    1023: ([('unsorted', 400), ('empty', 1), ('sorted', 622)], None),
    1024: ([('unsorted', 400), ('empty', 1), ('sorted', 623)], None),
    1025: ([('unsorted', 500), ('empty', 1), ('wide', 2), ('sorted', 522)], 'inside'),
    2048: ([('unsorted', 600), ('empty', 1), ('sorted', 423), ('unsorted', 1024)], 'first'),
    2049: ([('unsorted', 600), ('empty', 1), ('sorted', 800), ('unsorted', 637), ('edges', 11)], 'skipped'),
}


@functools.lru_cache(maxsize=None)
def edge_pack_regions(n_cands):
  """-> PackCase(regions holding exactly n_cands candidates together, what lies on the edge)."""
  layout, edge = _PACK_LAYOUT[n_cands]
  regions, first = [], 0
  for k, (kind, count) in enumerate(layout):
    if kind == 'empty':
      region = PC.empty_region()
    elif kind == 'wide':
      region = wide_region()
    elif kind == 'edges':
      region = PC.edges_region()
    else:
      forced = {}
      for c, window in ((SCAN_STEP - 2, True), (SCAN_STEP - 1, edge != 'skipped'), (SCAN_STEP, True)):
        if edge and first <= c < first + count:
          forced[c - first] = window
      region = _small_region(20261105 + 10 * n_cands + k, '%s%d_' % (kind[0], k), count, kind == 'unsorted', forced)
    assert len(region.candidates) == count, (kind, count)
    regions.append(region)
    first += count
  assert first == n_cands
  return PackCase(tuple(regions), edge)


@functools.lru_cache(maxsize=None)
def pack_expected(n_cands, use_groups):
  return PC.expected(list(edge_pack_regions(n_cands).regions), use_groups)


def pack_candidates(case):
  """[(region, candidate)] in batch order."""
  return [(r, c) for r in case.regions for c in r.candidates]


# ---------------------------------------------------------------- candidates / gVCF: regions
RegionsCase = collections.namedtuple('RegionsCase', 'ref spans reads kinds slots overflow_at')
REGION_KINDS = ('snp', 'indels', 'readless', 'quiet')
_REGIONS_AT = 3000                     # in front of it lies the stretch the noisy region of the overflow case uses


@functools.lru_cache(maxsize=None)
def edge_regions(n, overflow_at=None):
  """Regions of at most 80 bases and at most 14 reads on one synthetic reference, cycling through: a quiet pile
  with one SNP (test_hip_candidates._quiet_reads' shape), a pile with an insertion and a deletion, a region with
  no reads, and reads without a candidate; spans, depths and the SNP's place vary from region to region, so
  sites, alleles and blocks per region differ and some regions contribute none.

  What the pack kernels step over is the regions of the device pass: plan_batch (csrc/allele_counter_plan.h) gives
  a region without reads no slot -- it takes the one-region path -- so a batch of 300 regions of which every fourth
  is readless launches 225 workgroups and never takes a second step.  `n` is therefore the number of regions WITH
  reads, exactly; the readless ones lie between them on top of it (`slots`: per region its index among the
  regions with reads, or -1), so region numbers and slot numbers differ from the third region on.
  `overflow_at`: the region with that slot is the noisy one of
  test_hip_candidates.test_events_beyond_the_first_guess, which leaves the batch and is counted alone while its
  records are still packed."""
  from tests import test_hip_candidates as HC
  rng = np.random.default_rng(20261106)
  n_regions = 4 * (n // 3) + n % 3                                            # three of four have reads; so has the last
  seq = ''.join('ACGT'[int(i)] for i in rng.integers(0, 4, size=_REGIONS_AT + 100 * n_regions))
  ref = HC._SeqRef(seq)                                                       # pylint: disable=protected-access
  spans, reads, kinds, slots = [], [], [], []
  n_slots = 0
  for k in range(n_regions):
    start = _REGIONS_AT + 100 * k + 10
    kind = REGION_KINDS[k % 4]
    span = (start - 5 - k % 6, start + 60 + k % 9)
    if kind != 'readless' and n_slots == overflow_at:
      kind, span, rs = 'noisy', (1000, 1400), HC._noisy_reads(ref)            # pylint: disable=protected-access
    elif kind == 'snp':
      at = start + 20 + k % 25
      rs = HC._pile(ref, 'ref', 6 + k % 5, start=start) + HC._pile(ref, 'alt', 4, start=start, edit=HC._sub_at(at, start))   # pylint: disable=protected-access
    elif kind == 'indels':
      rs = (HC._pile(ref, 'ref', 8 - k % 3, start=start) +                    # pylint: disable=protected-access
            HC._indel_reads(ref, 'ins', 3, start + 20, inserted='TT', start=start) +   # pylint: disable=protected-access
            HC._indel_reads(ref, 'del', 3, start + 40, deleted=2, start=start))        # pylint: disable=protected-access
    elif kind == 'readless':
      rs = []
    else:
      rs = HC._pile(ref, 'ref', 3 + k % 9, start=start)                       # pylint: disable=protected-access
    assert kind == 'noisy' or (span[1] - span[0] <= 80 and len(rs) <= 14)
    spans.append(span)
    reads.append(tuple(rs))
    kinds.append(kind)
    slots.append(n_slots if rs else -1)
    n_slots += bool(rs)
  assert n_slots == n and slots[-1] == n - 1
  return RegionsCase(ref, tuple(spans), tuple(reads), tuple(kinds), tuple(slots), overflow_at)


def region_of_slot(case, slot):
  return case.slots.index(slot)


def counters(case, positions=None, track=False, lo=0, hi=None):
  """Fresh AlleleCounters for regions lo .. hi-1 (`positions`: one list per returned counter, or None)."""
  from deepvariant_amd import allelecounter as A
  out = []
  for k in range(lo, len(case.spans) if hi is None else hi):
    s, e = case.spans[k]
    c = A.AlleleCounter(case.ref, 'c', s, e, candidate_positions=positions[k - lo] if positions else (),
                        min_mapping_quality=10, min_base_quality=10, track_ref_reads=track)
    for r in case.reads[k]:
      c.add(r)
    out.append(c)
  return out
