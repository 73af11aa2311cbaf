"""Host mirror of the reference's AlleleCounter over the C ABI (`dv_count_alleles`).

  AlleleCounter(ref, range, candidate_positions, options)   deepvariant/allelecounter.h:206-518
  .add(read, sample) / .counts() / .summary_counts()        deepvariant/allelecounter.cc:873-1008
  sum_allele_counts / total_allele_counts                    deepvariant/allelecounter.cc:78-203

track_ref_reads + candidate_positions (the two-pass scheme of make_examples_core.py:2880-2932) are
supported: at candidate positions the reference-supporting reads come back by name too.
The reference adds reads one by one on the CPU; here `add` only queues them and the first
call that needs results packs the queue (packing.ReadTable) and counts the whole region in
ONE kernel launch (deepvariant_amd/csrc/allele_counter.hip).  There is no CPU path.
normalize_cigar restates AlleleCounter::NormalizeCigar (:777-845) for --normalize_reads.
gvcf_blocks / run_batch(gvcf=...) add the reference's VariantCaller.make_gvcfs(summary_counts())
(deepvariant/variant_caller.py), computed on the device from the same counts
(deepvariant_amd/csrc/gvcf.hip); variant_calling.VariantCaller.make_gvcfs is its host restatement.
candidates / candidate_positions / run_batch(call=...) add the reference's VariantCaller::CallsFromAlleleCounter
and CallPositionsFromAlleleCounts (variant_calling.cc:365-382, variant_calling_multisample.cc:940-1004) in the same way
(deepvariant_amd/csrc/candidates.hip): the device groups the events into alleles and applies the thresholds, and
only the candidate positions' alleles are built here; variant_calling.VariantCaller is the host restatement.
"""
from __future__ import annotations

import collections
import ctypes as C
import os
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from deepvariant_amd import _lib
from deepvariant_amd import dv_types as T
from deepvariant_amd import packing

REFERENCE, SUBSTITUTION, INSERTION, DELETION, SOFT_CLIP = 1, 2, 3, 4, 5   # AlleleType
_EVENT_DTYPE = np.dtype([('position', '<i4'), ('read', '<u4'), ('read_offset', '<u4'),
                         ('length_type', '<u4')])        # dv_allele_event: length | type << 28 | low quality << 31
GVCF_BLOCK_DTYPE = np.dtype([('start', '<i8'), ('end', '<i8'), ('likelihoods', '<f8', (3,)), ('gq', '<i4'),
                             ('min_dp', '<i4'), ('med_dp', '<i4'), ('ref_base', 'u1'), ('has_valid_gl', 'u1'),
                             ('reserved', 'u1', (2,))])   # dv_gvcf_block
CANDIDATE_SITE_DTYPE = np.dtype([('offset', '<i4'), ('ref_count', '<i4'), ('total', '<i4'), ('first_allele', '<i4'),
                                 ('n_alleles', '<i4')])    # dv_candidate_site
CANDIDATE_ALLELE_DTYPE = np.dtype([('length_type', '<u4'), ('count', '<i4'), ('read', '<u4'),
                                   ('read_offset', '<u4')])   # dv_candidate_allele
EVENT_UNCALLED, EVENT_OVERWRITTEN = -1, -2                  # DV_CANDIDATE_EVENT_*


BatchStats = collections.namedtuple('BatchStats', 'regions regions_batched regions_alone count_launches count_workgroups')


def count_one_launch() -> bool:
  """DV_COUNT_ONE_LAUNCH=1: every batch entry point (`run_batch` in all its forms) counts its batched regions in one
  kernel launch instead of one launch per region.  The library reads the switch at each call; results do not depend
  on it.  Off by default."""
  return os.environ.get('DV_COUNT_ONE_LAUNCH', '') == '1'


def last_batch_stats() -> BatchStats:
  """dv_count_batch_last_stats of the calling thread: how the last batch call's counting was launched."""
  s = _lib.DvCountBatchStats()
  _lib.check(_lib.lib().dv_count_batch_last_stats(C.byref(s)))
  return BatchStats(s.regions, s.regions_batched, s.regions_alone, s.count_launches, s.count_workgroups)


class Allele:
  """deepvariant.proto Allele: bases, type, count, is_low_quality."""

  def __init__(self, bases: str, type_: int, count: int = 1, is_low_quality: bool = False):
    self.bases, self.type, self.count, self.is_low_quality = bases, type_, count, is_low_quality

  def __repr__(self):
    return 'Allele(%r, %d, %d%s)' % (self.bases, self.type, self.count, ', low quality' if self.is_low_quality else '')


class AlleleCount:
  """deepvariant.proto AlleleCount (the fields the candidate caller reads)."""

  def __init__(self, reference_name: str, position: int, ref_base: str):
    self.position = T.Position(reference_name, position, False)
    self.ref_base = ref_base
    self.ref_supporting_read_count = 0
    self.read_alleles: Dict[str, Allele] = {}
    self.track_ref_reads = False


class CandidateSite(AlleleCount):
  """One position the device caller selected alternate alleles at (AlleleCounter.candidates): the
  AlleleCount fields, plus `selected` (the selected Alleles with their counts, in SumAlleleCounts
  order) and `total` (TotalAlleleCounts).  read_alleles is complete and in the map's order, but only
  the reads that support a selected allele (or the reference) carry a text: the others' bases are None."""

  def __init__(self, reference_name: str, position: int, ref_base: str):
    super().__init__(reference_name, position, ref_base)
    self.selected: List[Allele] = []
    self.total = 0


def sum_allele_counts(allele_count: AlleleCount, include_low_quality: bool = False) -> List[Allele]:
  """SumAlleleCounts (:78-117): std::map order = (bases, type) ascending, then the synthetic
  reference allele."""
  sums: Dict[Tuple[str, int], int] = {}
  for allele in allele_count.read_alleles.values():
    if include_low_quality or not allele.is_low_quality:
      k = (allele.bases, allele.type)
      sums[k] = sums.get(k, 0) + 1
  out = [Allele(b, t, n) for (b, t), n in sorted(sums.items())]
  if allele_count.ref_supporting_read_count > 0 and not getattr(allele_count, 'track_ref_reads', False):
    out.append(Allele(allele_count.ref_base, REFERENCE, allele_count.ref_supporting_read_count))
  return out


def total_allele_counts(allele_count: AlleleCount, include_low_quality: bool = False) -> int:
  """TotalAlleleCounts (:165-176)."""
  n = sum(1 for a in allele_count.read_alleles.values()
          if (not a.is_low_quality or include_low_quality) and a.type != REFERENCE)
  return n + allele_count.ref_supporting_read_count


def phasing_arrays_from_events(ev, words, sites, alleles, key_ids, start, bases, seq_off, window, w0):
  """The pure array step of AlleleCounter.phasing_arrays: the device caller's sites, selected alleles and event
  words plus the counter's events -> (candidates, alleles, bases, support_reads, support_low_quality) in
  direct_phasing's record layouts, offsets relative to these arrays.

  Per site, as VariantCaller._add_supporting_reads followed by DirectPhasing.phase build them: read_alleles is a map
  by read key in the order the keys first appear among the site's events, each key with its last ("standing") event;
  one is_ref entry from the standing REFERENCE events, then one entry per selected allele in the order the standing
  events first name it; events with the "uncalled" word are UNCALLED_ALLELE and left out.  A read index is the LAST
  row that has the event's key (`key_ids`: key number per row, None = all distinct).  start / end are the variant's:
  the reference bases grow with the longest selected deletion, and an allele's bases are the variant's alternate:
  substitutions byte for byte; an insertion or deletion only has the right length, which is all the candidate filter
  reads of a site it refuses."""
  from deepvariant_amd import direct_phasing as dp     # pylint: disable=g-import-not-at-top
  n_sites = len(sites)
  lo = np.searchsorted(ev['position'], sites['offset'], 'left')
  hi = np.searchsorted(ev['position'], sites['offset'], 'right')
  counts = hi - lo
  before = np.cumsum(counts) - counts
  site_of = np.repeat(np.arange(n_sites), counts)
  idx = np.arange(int(counts.sum())) - np.repeat(before, counts) + np.repeat(lo, counts)
  e, word = ev[idx], words[idx].astype(np.int64)
  packed = e['length_type']
  kind, low = (packed >> 28) & 7, (packed >> 31).astype(np.uint8)
  row = e['read'].astype(np.int64)
  order = np.arange(len(idx))                     # read_alleles order: where the event's key first appears in the site
  read_index = row
  if key_ids is not None:
    key_ids = np.asarray(key_ids, np.int64)
    n_keys = int(key_ids.max()) + 1 if len(key_ids) else 1
    _, first, inverse = np.unique(site_of * n_keys + key_ids[row], return_index=True, return_inverse=True)
    order = first[inverse]
    last_row = np.zeros(n_keys, np.int64)
    last_row[key_ids] = np.arange(len(key_ids))   # a later row with the same key wins
    read_index = last_row[key_ids[row]]
  kept = np.nonzero((word != EVENT_OVERWRITTEN) & ((kind == REFERENCE) | (word >= 0)))[0]
  stride = int(sites['n_alleles'].max()) + 1 if n_sites else 1
  slot = np.where(kind[kept] == REFERENCE, 0, 1 + word[kept])
  entries, entry_of = np.unique(site_of[kept] * stride + slot, return_inverse=True)
  first_named = np.full(len(entries), np.iinfo(np.int64).max)
  np.minimum.at(first_named, entry_of, order[kept])
  entry_site, entry_slot = entries // stride, entries % stride
  by_order = np.lexsort((first_named, entry_slot != 0, entry_site))     # the is_ref entry first, then as first named
  rank = np.empty(len(entries), np.int64)
  rank[by_order] = np.arange(len(entries))
  final = np.lexsort((order[kept], rank[entry_of]))
  support_reads = np.ascontiguousarray(read_index[kept][final], np.int32)
  support_low = np.ascontiguousarray(low[kept][final], np.uint8)
  n_support = np.bincount(entry_of, minlength=len(entries))[by_order]
  entry_site, entry_slot = entry_site[by_order], entry_slot[by_order]

  # the variant's reference span: one base, or the longest selected deletion behind its anchor
  a_packed = alleles['length_type']
  a_len, a_kind = (a_packed & 0x0fffffff).astype(np.int64), (a_packed >> 28) & 7
  a_site = np.repeat(np.arange(n_sites), sites['n_alleles'])
  a_index = np.arange(len(a_site)) - np.repeat(np.cumsum(sites['n_alleles']) - sites['n_alleles'], sites['n_alleles']) + \
      np.repeat(sites['first_allele'], sites['n_alleles'])
  span = np.ones(n_sites, np.int64)
  np.maximum.at(span, a_site, np.where(a_kind[a_index] == DELETION, 1 + a_len[a_index], 1))
  is_ref = entry_slot == 0
  chosen = sites['first_allele'][entry_site] + np.maximum(entry_slot - 1, 0)      # the entry's selected allele
  c_kind, c_len = a_kind[chosen], a_len[chosen]
  width = span[entry_site]
  bases_len = np.where(is_ref, 0, np.where(c_kind == INSERTION, width + c_len,
                                           np.where(c_kind == DELETION, width - c_len, width)))
  bases_off = np.cumsum(bases_len) - bases_len
  blob = np.full(int(bases_len.sum()), ord('N'), np.uint8)
  substitution = ~is_ref & (c_kind == SUBSTITUTION)
  s0 = seq_off[alleles['read'][chosen]].astype(np.int64) + alleles['read_offset'][chosen]
  blob[bases_off[substitution]] = bases[s0[substitution]]
  for k in np.nonzero(substitution & (width > 1))[0].tolist():       # a substitution beside a deletion: its reference tail
    anchor = start + int(sites['offset'][entry_site[k]]) - w0
    tail = np.frombuffer(window[anchor + 1:anchor + int(width[k])], np.uint8)
    blob[bases_off[k] + 1:bases_off[k] + 1 + len(tail)] = tail

  allele_records = np.zeros(len(entries), dp.ALLELE_DTYPE)
  allele_records['bases_off'], allele_records['bases_len'], allele_records['is_ref'] = bases_off, bases_len, is_ref
  allele_records['support_off'], allele_records['n_support'] = np.cumsum(n_support) - n_support, n_support
  per_site = np.bincount(entry_site, minlength=n_sites)
  candidates = np.zeros(n_sites, dp.CANDIDATE_DTYPE)
  candidates['start'] = start + sites['offset'].astype(np.int64)
  candidates['end'] = candidates['start'] + span
  candidates['allele_off'], candidates['n_alleles'] = np.cumsum(per_site) - per_site, per_site
  return candidates, allele_records, blob, support_reads, support_low


class AlleleCounter:
  def __init__(self, ref_reader, reference_name: str, start: int, end: int,
               candidate_positions: Sequence[int] = (), min_mapping_quality: int = 0,
               min_base_quality: int = 0, keep_legacy_behavior: bool = False,
               full_range: Optional[Tuple[int, int]] = None, track_ref_reads: bool = False):
    self._track_ref_reads = bool(track_ref_reads)
    self._candidate_positions = np.ascontiguousarray(sorted(int(p) for p in candidate_positions), np.int64)
    self._ref = ref_reader
    self._contig, self._start, self._end = reference_name, int(start), int(end)
    self._reads_start = min(self._start, full_range[0]) if full_range else self._start
    self._reads_end = max(self._end, full_range[1]) if full_range else self._end
    self._opt = (int(min_mapping_quality), int(min_base_quality), bool(keep_legacy_behavior))
    self._reads: List = []
    self._table: Optional[packing.ReadTable] = None
    self._counts: Optional[List[AlleleCount]] = None
    self._alleles: Optional[Dict[int, Dict[str, Allele]]] = None
    self._events = None
    self._event_ctx = None
    self._n_counted = 0
    self._gvcf = None            # (GvcfOptions.key(), dv_gvcf_block records) of the last gVCF pass
    self._cand = None            # (CandidateOptions.key(), sites, alleles, event words) of the last candidate pass
    self._cand_positions = None  # (CandidateOptions.key(), offsets) of the last positions-only pass
    self._windows = None         # (window key, starts, ends, candidate mask, scores) of the last window pass

  # ---- the reference's interface
  def interval_length(self) -> int:
    return self._end - self._start

  def interval_start(self) -> int:
    return self._start

  def add(self, read, sample: str = ''):
    if self._table is not None:
      raise ValueError('reads were handed over as a packed table; add() cannot be mixed in')
    self._reads.append(read)
    self._counts = self._alleles = self._events = self._gvcf = self._cand = self._cand_positions = None
    self._windows = None

  def add_table(self, table: packing.ReadTable):
    """All reads of the region at once, already packed (packing.ReadTable.from_bam / from_reads)."""
    if self._reads:
      raise ValueError('add() was used; add_table() cannot be mixed in')
    self._table = table
    self._counts = self._alleles = self._events = self._gvcf = self._cand = self._cand_positions = None
    self._windows = None

  def _ensure(self):
    if self._events is None:
      self._run()

  def _count_at(self, i: int) -> AlleleCount:
    self._build_alleles()
    c = AlleleCount(self._contig, self._start + i, self._interval_ref[i])
    c.ref_supporting_read_count = int(self._ref_counts[i])
    c.track_ref_reads = self._track_ref_reads
    c.read_alleles = self._alleles.get(i, {})
    return c

  def counts(self) -> List[AlleleCount]:
    """Counts(): one AlleleCount per position of the interval."""
    self._ensure()
    if self._counts is None:
      self._counts = [self._count_at(i) for i in range(len(self._ref_counts))]
    return self._counts

  def counts_with_read_alleles(self) -> List[AlleleCount]:
    """Only the positions some read left a non-reference (or tracked reference) allele at, in
    order -- all a candidate caller or window selector has to look at: a position without read
    alleles has no alternate allele to select."""
    self._ensure()
    self._build_alleles()
    return [self._count_at(i) for i in sorted(self._alleles)]

  def counts_with_alt_support(self, min_count: int) -> List[AlleleCount]:
    """The positions at which at least `min_count` reads left a good-quality allele that is
    neither the reference nor a soft clip, in order.  An alternate allele's count is at most that
    number, so a candidate caller whose thresholds ask for `min_count` reads per allele
    (IsGoodAltAllele, variant_calling_multisample.cc:232-238) finds every candidate among them --
    one position in twenty of the ones `counts_with_read_alleles` returns on 30x Illumina data,
    where most read alleles are lone sequencing errors.  The AlleleCounts are complete (all read
    alleles of the position, low-quality ones included); only those positions' Allele objects
    are built."""
    self._ensure()
    ev = self._events
    if not len(ev):
      return []
    packed = ev['length_type']
    kind = (packed >> 28) & 7
    n = self._end - self._start
    good = ((packed >> 31) == 0) & (kind != REFERENCE) & (kind != SOFT_CLIP) & (ev['position'] >= 0) & (ev['position'] < n)
    per_position = np.bincount(ev['position'][good], minlength=n) if good.any() else np.zeros(n, np.int64)
    wanted = np.nonzero(per_position >= max(1, int(min_count)))[0]
    if not len(wanted):
      return []
    if self._alleles is not None:
      return [self._count_at(int(i)) for i in wanted.tolist()]
    alleles = self._alleles_of(np.nonzero(np.isin(ev['position'], wanted))[0])
    out = []
    for i in wanted.tolist():
      c = AlleleCount(self._contig, self._start + i, self._interval_ref[i])
      c.ref_supporting_read_count = int(self._ref_counts[i])
      c.track_ref_reads = self._track_ref_reads
      c.read_alleles = alleles.get(i, {})
      out.append(c)
    return out

  def ref_supporting_read_counts(self) -> np.ndarray:
    self._ensure()
    return self._ref_counts

  def n_counted_reads(self) -> int:
    self._ensure()
    return self._n_counted

  def summary_counts(self, left_padding: int = 0, right_padding: int = 0):
    """SummaryCounts (:986-1008) -> [(reference_name, position, ref_base, ref_supporting_read_count,
    total_read_count)]."""
    counts = self.counts()
    if left_padding < 0 or right_padding < 0 or left_padding + right_padding >= len(counts):
      raise ValueError('Check failed: left_padding + right_padding < counts_.size()')
    return [(self._contig, c.position.position, c.ref_base, c.ref_supporting_read_count, total_allele_counts(c))
            for c in counts[left_padding:len(counts) - right_padding]]

  # ---- the launch
  def _request(self):
    """-> (packed batch, options struct, the objects they point into, (table, window, w0, interval_ref))."""
    table = self._table if self._table is not None else packing.ReadTable.from_reads(self._reads)
    n_contig = self._ref.n_bases(self._contig)
    # reference window: the reads interval plus room for the longest deletion anchored inside it
    ops, lens = table.cigar & 15, table.cigar >> 4
    margin = int(lens[ops == 3].max()) + 1 if (ops == 3).any() else 1
    w0 = max(0, self._reads_start - 1)
    w1 = min(n_contig, self._reads_end + margin)
    window = self._ref.get_bases(self._contig, w0, w1).encode()
    interval_ref = self._ref.get_bases(self._contig, self._start, self._end)
    opt = _lib.DvAlleleCounterOptions(
        self._start, self._end, self._reads_start, self._reads_end, window, w0, len(window), n_contig,
        self._opt[0], self._opt[1], int(self._opt[2]), int(self._track_ref_reads),
        self._candidate_positions.ctypes.data if len(self._candidate_positions) else None,
        len(self._candidate_positions))
    b, keep = packing.PackedBatch(table=table, width=3).to_ctypes()
    return b, opt, keep, (table, window, w0, interval_ref)

  def _take(self, handle, ctx) -> None:
    """Copies the result out of a dv_allele_counts handle and frees it."""
    table, window, w0, interval_ref = ctx
    lib = _lib.lib()
    try:
      refc = C.POINTER(C.c_int32)()
      events = C.POINTER(_lib.DvAlleleEvent)()
      n_events, n_counted = C.c_uint32(), C.c_int32()
      length = lib.dv_allele_counts_arrays(handle, C.byref(refc), C.byref(events), C.byref(n_events),
                                           C.byref(n_counted))
      self._interval_ref = interval_ref
      self._ref_counts = np.ctypeslib.as_array(refc, shape=(length,)).copy() if length else np.zeros(0, np.int32)
      n_ev = int(n_events.value)
      ev = (np.ctypeslib.as_array(C.cast(events, C.POINTER(C.c_uint8)), shape=(n_ev * 16,)).view(_EVENT_DTYPE).copy()
            if n_ev else np.zeros(0, _EVENT_DTYPE))
      # the Allele objects (texts cut out of the reads / the reference) are built on demand: the
      # window selector's default model only needs the events' footprints (variant_read_window_counts)
      self._events, self._event_ctx = ev, (table, window, w0)
      self._alleles, self._counts, self._n_counted = None, None, int(n_counted.value)
    finally:
      lib.dv_allele_counts_free(handle)

  def _run(self):
    b, opt, keep, ctx = self._request()
    handle = C.c_void_p()
    _lib.check(_lib.lib().dv_count_alleles(C.byref(b), C.byref(opt), C.byref(handle), None))
    del keep
    self._take(handle, ctx)

  @staticmethod
  def run_batch(counters: Sequence['AlleleCounter'], gvcf=None, call=None, windows=None,
                window_debug: bool = False) -> None:
    """Counts for several counters (a batch of calling regions, each with its reads added) in ONE
    dv_count_alleles_batch call: one upload, kernels back to back, two synchronisations for the
    whole batch.  Afterwards every counter answers as if it had counted alone.  With `gvcf`
    (variant_calling.GvcfOptions) the gVCF blocks of every counter are computed in the same device
    pass (dv_count_alleles_gvcf_batch) and `gvcf_blocks(gvcf)` answers without another launch.  With
    `call` (variant_calling.CandidateOptions) so are the candidates (dv_call_candidates_batch):
    `candidates(call)` / `candidate_positions(call)` then answer without another launch; a
    positions-only pass leaves the counters uncounted.  With `windows` (the realigner's
    WindowSelectorOptions) the realigner's windows are selected in the same way
    (dv_select_windows_batch): `windows(options)` then answers without another launch, nothing but the
    windows comes home and the counters stay uncounted (`window_debug`: the candidate mask and the scores
    come too, for `windows(options, want_debug=True)`)."""
    if windows is not None:
      if gvcf is not None or call is not None:
        raise ValueError('the window pass runs on its own')
      key = _window_key(windows, window_debug)
      AlleleCounter._run_window_batch([c for c in counters if not c._has_windows(key)], windows, window_debug)   # pylint: disable=protected-access
      return
    if call is not None:
      todo = [c for c in counters if not c._has_candidates(call) or                   # pylint: disable=protected-access
              (gvcf is not None and (c._gvcf is None or c._gvcf[0] != gvcf.key()))]   # pylint: disable=protected-access
      AlleleCounter._run_call_batch(todo, call, gvcf)
      return
    if gvcf is not None:
      AlleleCounter._run_gvcf_batch(
          [c for c in counters if c._gvcf is None or c._gvcf[0] != gvcf.key()], gvcf)   # pylint: disable=protected-access
      return
    todo = [c for c in counters if c._events is None]      # pylint: disable=protected-access
    if not todo:
      return
    if len(todo) == 1:
      todo[0]._run()                                       # pylint: disable=protected-access
      return
    requests = [c._request() for c in todo]                # pylint: disable=protected-access
    n = len(todo)
    batches = (C.c_void_p * n)(*[C.addressof(r[0]) for r in requests])
    options = (C.c_void_p * n)(*[C.addressof(r[1]) for r in requests])
    handles = (C.c_void_p * n)()
    _lib.check(_lib.lib().dv_count_alleles_batch(n, batches, options, handles, None))
    taken = 0
    try:
      for c, r, h in zip(todo, requests, handles):
        taken += 1                                         # _take frees its handle, also when it raises
        c._take(C.c_void_p(h), r[3])                       # pylint: disable=protected-access
    finally:
      for h in list(handles)[taken:]:                      # a failure part-way: the rest is not leaked
        if h:
          _lib.lib().dv_allele_counts_free(C.c_void_p(h))

  @staticmethod
  def _run_gvcf_batch(todo: Sequence['AlleleCounter'], gvcf) -> None:
    if not todo:
      return
    requests = [c._request() for c in todo]                # pylint: disable=protected-access
    n = len(todo)
    keys = [AlleleCounter._read_key_ids(r[3][0].keys) for r in requests]
    table = gvcf.table()
    opt = _lib.DvGvcfOptions(gvcf.p_error, gvcf.max_gq, gvcf.gq_resolution, gvcf.max_cache_coverage,
                             int(gvcf.include_med_dp), gvcf.left_padding, gvcf.right_padding,
                             table.ctypes.data, len(table))
    batches = (C.c_void_p * n)(*[C.addressof(r[0]) for r in requests])
    options = (C.c_void_p * n)(*[C.addressof(r[1]) for r in requests])
    key_ptrs = (C.c_void_p * n)(*[k.ctypes.data if k is not None else None for k in keys])
    handles = (C.c_void_p * n)()
    blocks = (C.c_void_p * n)()
    lib = _lib.lib()
    _lib.check(lib.dv_count_alleles_gvcf_batch(n, batches, options, key_ptrs, C.byref(opt), handles, blocks, None))
    taken = 0
    try:
      for c, r, h, b in zip(todo, requests, handles, blocks):
        taken += 1                                         # both handles are freed below, also on an error
        try:
          records = C.POINTER(_lib.DvGvcfBlock)()
          nb = int(lib.dv_gvcf_blocks_arrays(C.c_void_p(b), C.byref(records)))
          # string_at: one copy, ~100x cheaper per call than np.ctypeslib.as_array on a pointer
          arr = (np.frombuffer(C.string_at(records, nb * GVCF_BLOCK_DTYPE.itemsize), GVCF_BLOCK_DTYPE)
                 if nb else np.zeros(0, GVCF_BLOCK_DTYPE))
        finally:
          lib.dv_gvcf_blocks_free(C.c_void_p(b))
        c._take(C.c_void_p(h), r[3])                       # pylint: disable=protected-access
        c._gvcf = (gvcf.key(), arr)                        # pylint: disable=protected-access
    finally:
      for h, b in list(zip(handles, blocks))[taken:]:
        if h:
          lib.dv_allele_counts_free(C.c_void_p(h))
        if b:
          lib.dv_gvcf_blocks_free(C.c_void_p(b))

  def _has_candidates(self, call) -> bool:
    if self._cand is not None and self._cand[0] == call.key():
      return True
    return bool(call.positions_only) and self._cand_positions is not None and self._cand_positions[0] == call.key()

  @staticmethod
  def _read_key_ids(names) -> Optional[np.ndarray]:
    """read_alleles is keyed by read key: reads that share one (supplementary alignments) are one key."""
    ids: Dict[str, int] = {}
    per_read = [ids.setdefault(name, len(ids)) for name in names]     # (np.unique on strings costs 100 us a region)
    return None if len(ids) == len(names) else np.ascontiguousarray(per_read, np.int32)

  @staticmethod
  def _run_call_batch(todo: Sequence['AlleleCounter'], call, gvcf=None) -> None:
    if not todo:
      return
    if call.positions_only and gvcf is not None:
      raise ValueError('a positions-only candidate pass has no gVCF records')
    requests = [c._request() for c in todo]                # pylint: disable=protected-access
    n = len(todo)
    keys = [AlleleCounter._read_key_ids(r[3][0].keys) for r in requests]
    copt = _lib.DvCandidateOptions(int(call.min_count_snps), int(call.min_count_indels), float(call.min_fraction_snps),
                                   float(call.min_fraction_indels), int(call.track_ref_reads), int(call.positions_only))
    gopt = None
    if gvcf is not None:
      table = gvcf.table()
      gopt = _lib.DvGvcfOptions(gvcf.p_error, gvcf.max_gq, gvcf.gq_resolution, gvcf.max_cache_coverage,
                                int(gvcf.include_med_dp), gvcf.left_padding, gvcf.right_padding,
                                table.ctypes.data, len(table))
    batches = (C.c_void_p * n)(*[C.addressof(r[0]) for r in requests])
    options = (C.c_void_p * n)(*[C.addressof(r[1]) for r in requests])
    key_ptrs = (C.c_void_p * n)(*[k.ctypes.data if k is not None else None for k in keys])
    handles, blocks, cands = (C.c_void_p * n)(), (C.c_void_p * n)(), (C.c_void_p * n)()
    lib = _lib.lib()
    _lib.check(lib.dv_call_candidates_batch(n, batches, options, key_ptrs, C.byref(copt),
                                            C.byref(gopt) if gopt is not None else None,
                                            None if call.positions_only else handles,
                                            blocks if gopt is not None else None, cands, None))
    taken = 0
    try:
      for c, r, h, b, d in zip(todo, requests, handles, blocks, cands):
        taken += 1                                         # this region's handles are freed below, also on an error
        try:
          sites, alleles, words = C.c_void_p(), C.c_void_p(), C.c_void_p()
          n_alleles, n_words = C.c_int32(), C.c_uint32()
          n_sites = int(lib.dv_candidates_arrays(C.c_void_p(d), C.byref(sites), C.byref(alleles), C.byref(n_alleles),
                                                 C.byref(words), C.byref(n_words)))

          def array(pointer, count, dtype):
            return (np.frombuffer(C.string_at(pointer, count * dtype.itemsize), dtype) if count
                    else np.zeros(0, dtype))
          site_arr = array(sites, n_sites, CANDIDATE_SITE_DTYPE)
          allele_arr = array(alleles, n_alleles.value, CANDIDATE_ALLELE_DTYPE)
          word_arr = array(words, n_words.value, np.dtype('<i4'))
          block_arr = None
          if gopt is not None:
            records = C.POINTER(_lib.DvGvcfBlock)()
            nb = int(lib.dv_gvcf_blocks_arrays(C.c_void_p(b), C.byref(records)))
            block_arr = array(records, nb, GVCF_BLOCK_DTYPE)
        finally:
          lib.dv_candidates_free(C.c_void_p(d))
          if b:
            lib.dv_gvcf_blocks_free(C.c_void_p(b))
        if call.positions_only:
          c._cand_positions = (call.key(), site_arr['offset'].astype(np.int64))   # pylint: disable=protected-access
          continue
        c._take(C.c_void_p(h), r[3])                       # pylint: disable=protected-access
        c._cand = (call.key(), site_arr, allele_arr, word_arr)   # pylint: disable=protected-access
        c._cand_positions = None                           # pylint: disable=protected-access
        if gopt is not None:
          c._gvcf = (gvcf.key(), block_arr)                # pylint: disable=protected-access
    finally:
      for h, b, d in list(zip(handles, blocks, cands))[taken:]:
        if h:
          lib.dv_allele_counts_free(C.c_void_p(h))
        if b:
          lib.dv_gvcf_blocks_free(C.c_void_p(b))
        if d:
          lib.dv_candidates_free(C.c_void_p(d))

  def _has_windows(self, key) -> bool:
    if self._windows is None:
      return False
    have = self._windows[0]
    # a pass that also brought the mask and the scores answers for one that did not
    return have == key or (not key[-1] and have[:-1] == key[:-1])

  @staticmethod
  def _run_window_batch(todo: Sequence['AlleleCounter'], config, want_debug: bool = False) -> None:
    if not todo:
      return
    requests = [c._request() for c in todo]                # pylint: disable=protected-access
    n = len(todo)
    keys = [AlleleCounter._read_key_ids(r[3][0].keys) for r in requests]
    key = _window_key(config, want_debug)
    wopt = _window_options_struct(config, want_debug)
    batches = (C.c_void_p * n)(*[C.addressof(r[0]) for r in requests])
    options = (C.c_void_p * n)(*[C.addressof(r[1]) for r in requests])
    key_ptrs = (C.c_void_p * n)(*[k.ctypes.data if k is not None else None for k in keys])
    handles = (C.c_void_p * n)()
    lib = _lib.lib()
    _lib.check(lib.dv_select_windows_batch(n, batches, options, key_ptrs, C.byref(wopt), None, handles, None))
    try:
      for c, h in zip(todo, handles):
        starts, ends, mask, scores = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
        n_windows = int(lib.dv_windows_arrays(C.c_void_p(h), C.byref(starts), C.byref(ends), C.byref(mask),
                                              C.byref(scores)))

        def array(pointer, count, dtype):
          return (np.frombuffer(C.string_at(pointer, count * np.dtype(dtype).itemsize), dtype) if count and pointer
                  else np.zeros(0, dtype))
        length = c._end - c._start                         # pylint: disable=protected-access
        mask_arr = score_arr = None
        if want_debug:
          words = array(mask, (length + 31) // 32, '<u4')
          mask_arr = np.unpackbits(words.view(np.uint8), bitorder='little')[:length].astype(bool)
          score_arr = array(scores, length, '<u4')
        c._windows = (key, array(starts, n_windows, '<i8'), array(ends, n_windows, '<i8'), mask_arr, score_arr)  # pylint: disable=protected-access
    finally:
      for h in handles:
        if h:
          lib.dv_windows_free(C.c_void_p(h))

  def windows(self, config, want_debug: bool = False):
    """select_windows' candidates and windows from the device (window_select.hip), for the realigner's
    WindowSelectorOptions `config`, over this counter's interval: -> (starts, ends) in contig coordinates, end
    exclusive, unclamped -- computed now unless run_batch(windows=...) already did with these options.  With
    `want_debug` -> (starts, ends, candidate mask [interval_length] bool, scores [interval_length] uint32: the
    float32 scores' bit patterns, or for the VARIANT_READS model the counts)."""
    key = _window_key(config, want_debug)
    if not self._has_windows(key):
      AlleleCounter._run_window_batch([self], config, want_debug)
    _, starts, ends, mask, scores = self._windows
    return (starts, ends, mask, scores) if want_debug else (starts, ends)

  def candidate_positions(self, call) -> List[int]:
    """CallPositionsFromAlleleCounts from the device: the absolute positions CallVariant will return a
    call for, in order.  Answers from a full candidate pass with the same thresholds when there was
    one; otherwise from a positions-only pass (run now unless run_batch(call=...) already did), which
    brings home the positions and nothing else."""
    if self._cand is not None and self._cand[0] == call.key():
      offsets = self._cand[1]['offset']
    else:
      if self._cand_positions is None or self._cand_positions[0] != call.key():
        AlleleCounter._run_call_batch([self], call.positions_form())
      offsets = self._cand_positions[1]
    return [self._start + int(o) for o in offsets]

  def candidates(self, call) -> List[CandidateSite]:
    """The positions at which the device caller selected alternate alleles (SelectAltAlleles), in
    order, each with what CallVariant needs -- computed now unless run_batch(call=...) already did
    with these thresholds.  Allele texts are cut for the selected alleles' representatives only;
    every other read allele of the site is known by the word the device left for its event."""
    if self._cand is None or self._cand[0] != call.key():
      AlleleCounter._run_call_batch([self], call.calls_form())
    _, sites, alleles, words = self._cand
    if not len(sites):
      return []
    ev = self._events
    table, window, w0 = self._event_ctx
    keys, bases, seq_off = table.keys, table.bases, table.read_seq_off
    first = np.searchsorted(ev['position'], sites['offset'], 'left').tolist()
    last = np.searchsorted(ev['position'], sites['offset'], 'right').tolist()
    out = []
    for site, lo, hi in zip(sites.tolist(), first, last):
      offset, ref_count, total, first_allele, n_alleles = site
      c = CandidateSite(self._contig, self._start + offset, self._interval_ref[offset])
      c.ref_supporting_read_count, c.total, c.track_ref_reads = ref_count, total, self._track_ref_reads
      selected = []
      for packed, count, read, read_offset in alleles[first_allele:first_allele + n_alleles].tolist():
        length_k, type_k = packed & 0x0fffffff, (packed >> 28) & 7
        s0 = int(seq_off[read]) + read_offset
        if type_k == SUBSTITUTION:
          text = chr(bases[s0])
        else:
          anchor = self._start + offset - w0              # the base the indel is anchored on
          prev = chr(bases[s0 - 1]) if read_offset > 0 else window[anchor:anchor + 1].decode()
          if type_k == DELETION:
            text = prev + window[anchor + 1:anchor + 1 + length_k].decode()
          else:
            text = prev + bytes(bases[s0:s0 + length_k]).decode()
        selected.append(Allele(text, type_k, count))
      c.selected = sorted(selected, key=lambda a: (a.bases, a.type))     # SumAlleleCounts' map order
      # read_alleles in the map's order: a key stands where it was first inserted, with its last value
      read_alleles: Dict[str, Optional[Allele]] = {}
      read_rows: Dict[str, int] = {}           # the event's row beside each entry: the row its value came from
      for (_, read, _, packed), word in zip(ev[lo:hi].tolist(), words[lo:hi].tolist()):
        key = keys[read]
        if word == EVENT_OVERWRITTEN:
          read_alleles.setdefault(key, None)
          read_rows.setdefault(key, read)
          continue
        read_rows[key] = read
        type_k, low = (packed >> 28) & 7, bool(packed >> 31)
        if type_k == REFERENCE:
          read_alleles[key] = Allele(c.ref_base, REFERENCE, 1, low)
        elif word >= 0:
          read_alleles[key] = Allele(selected[word].bases, type_k, 1, low)
        else:
          read_alleles[key] = Allele(None, type_k, 1, low)
      c.read_alleles = read_alleles
      c.read_rows = read_rows
      out.append(c)
    return out

  def phasing_arrays(self, call):
    """What read phasing reads of this counter's sites, as arrays (direct_phasing.phase_arrays' region layout
    without n_reads: candidates, alleles, bases, support_reads, support_low_quality) -- the lists
    DirectPhasing.phase builds from the calls of `candidates(call)`, with no Read, call or name made.  Read indices
    are rows of the counter's table.  Needs the candidate pass with track_ref_reads (run now unless
    run_batch(call=...) already did)."""
    if self._cand is None or self._cand[0] != call.key():
      AlleleCounter._run_call_batch([self], call.calls_form())
    _, sites, alleles, words = self._cand
    table, window, w0 = self._event_ctx
    return phasing_arrays_from_events(self._events, words, sites, alleles, AlleleCounter._read_key_ids(table.keys),
                                      self._start, table.bases, table.read_seq_off, window, w0)

  def gvcf_block_array(self, gvcf) -> np.ndarray:
    """The device's gVCF records of this counter (GVCF_BLOCK_DTYPE; MED_DP -1 unless asked for),
    computed now unless run_batch(gvcf=...) already did with these options."""
    if self._gvcf is None or self._gvcf[0] != gvcf.key():
      AlleleCounter._run_gvcf_batch([self], gvcf)
    return self._gvcf[1]

  def gvcf_blocks(self, gvcf) -> List[T.Variant]:
    """VariantCaller.make_gvcfs(self.summary_counts(left_padding, right_padding), include_med_dp)
    from the device: one Variant per reference block (variant_calling.gvcf_record)."""
    from deepvariant_amd import variant_calling          # pylint: disable=g-import-not-at-top (import cycle)
    return [variant_calling.gvcf_record(self._contig, b['start'], b['end'], chr(b['ref_base']),
                                        b['likelihoods'].tolist(), b['gq'], b['min_dp'],
                                        int(b['med_dp']) if gvcf.include_med_dp else None,
                                        bool(b['has_valid_gl']), gvcf.sample_name)
            for b in self.gvcf_block_array(gvcf)]

  def _build_alleles(self):
    if self._alleles is not None:
      return
    self._alleles, self._counts = self._alleles_of(None), None

  def _alleles_of(self, rows) -> Dict[int, Dict[str, Allele]]:
    """{position offset: {read key: Allele}} of the events `rows` (indices, ascending; None = all)."""
    ev = self._events if rows is None else self._events[rows]
    table, window, w0 = self._event_ctx
    seq_off = table.read_seq_off
    bases = table.bases
    keys = table.keys
    s0_all = seq_off[ev['read']].astype(np.int64) + ev['read_offset']
    alleles: Dict[int, Dict[str, Allele]] = {}
    for k, (position, read, read_offset, packed) in enumerate(ev.tolist()):
      length_k, type_k, low = packed & 0x0fffffff, (packed >> 28) & 7, packed >> 31
      s0 = int(s0_all[k])
      if type_k == SUBSTITUTION or type_k == REFERENCE:
        text = chr(bases[s0])
      else:
        anchor = self._start + position - w0              # the base the indel is anchored on
        prev = chr(bases[s0 - 1]) if read_offset > 0 else window[anchor:anchor + 1].decode()
        if type_k == DELETION:
          text = prev + window[anchor + 1:anchor + 1 + length_k].decode()
        else:
          text = prev + bytes(bases[s0:s0 + length_k]).decode()
      # a later read with the same key overwrites (read_alleles is a map keyed by ReadKey)
      alleles.setdefault(position, {})[keys[read]] = Allele(text, type_k, 1, bool(low))
    return alleles

  def variant_read_window_counts(self, min_allele_support: int = 0, strict_insertion_filter: bool = False):
    """VariantReadsWindowSelectorCandidates (window_selector.cc:101-141) straight from the events:
    per position of the interval, the number of reads whose non-reference allele covers it
    (substitution: its base; insertion / soft clip of n bases anchored at i: [i + 1 - n, i + 1 + n);
    deletion: [i + 1, i + 1 + n)).  Every read allele counts once whatever it is grouped with, so
    as long as no allele is filtered by its count (min_allele_support <= 1, no strict insertion
    filter) the sum over alleles of count x footprint is the sum over events of their footprint.
    With min_allele_support > 1 the events are grouped into alleles first -- by (position, type,
    text), the text of a substitution being its base, that of the few indel / clip events cut out
    as `_build_alleles` does -- and the events of alleles seen in fewer reads are dropped.
    -> int64[interval_length], or None when the strict insertion filter needs allele totals."""
    if strict_insertion_filter:
      return None
    self._ensure()
    n = self._end - self._start
    ev = self._events
    out = np.zeros(n + 1, np.int64)
    if not len(ev):
      return out[:n]
    packed = ev['length_type']
    length = (packed & 0x0fffffff).astype(np.int64)
    kind = (packed >> 28) & 7
    low = (packed >> 31).astype(bool)
    pos = ev['position'].astype(np.int64)
    # read_alleles is a map keyed by the read's name/number: of two events of one key at one
    # position the later one stands (supplementary alignments share their key)
    table = self._event_ctx[0]
    if len(set(table.keys)) != len(table.keys):
      key_id = np.unique(np.array(table.keys), return_inverse=True)[1][ev['read']]
      composite = pos * (int(key_id.max()) + 1) + key_id
      last = len(ev) - 1 - np.unique(composite[::-1], return_index=True)[1]
      keep = np.zeros(len(ev), bool)
      keep[last] = True
    else:
      keep = np.ones(len(ev), bool)
    keep &= ~low & (kind != REFERENCE)
    if min_allele_support > 1 and keep.any():
      _, window, w0 = self._event_ctx
      bases, seq_off = table.bases, table.read_seq_off
      s0_all = seq_off[ev['read']].astype(np.int64) + ev['read_offset']
      ident = np.zeros(len(ev), np.int64)
      sub = kind == SUBSTITUTION
      ident[sub] = bases[np.minimum(s0_all[sub], max(len(bases) - 1, 0))] if len(bases) else 0
      texts: Dict[bytes, int] = {}
      for k in np.nonzero(keep & ~sub)[0].tolist():
        s0, ln = int(s0_all[k]), int(length[k])
        anchor = self._start + int(pos[k]) - w0
        prev = bytes(bases[s0 - 1:s0]) if int(ev['read_offset'][k]) > 0 else window[anchor:anchor + 1]
        text = prev + (window[anchor + 1:anchor + 1 + ln] if kind[k] == DELETION else bytes(bases[s0:s0 + ln]))
        ident[k] = 256 + texts.setdefault(text, len(texts))
      m = 257 + len(texts)
      key = ((pos * 8 + kind.astype(np.int64)) * m + ident)[keep]
      _, inv, cnt = np.unique(key, return_inverse=True, return_counts=True)
      kept_rows = np.nonzero(keep)[0]
      keep = np.zeros(len(ev), bool)
      keep[kept_rows[cnt[inv] >= min_allele_support]] = True
    lo = np.where(kind == SUBSTITUTION, pos, np.where(kind == DELETION, pos + 1, pos + 1 - length))
    hi = np.where(kind == SUBSTITUTION, pos + 1, pos + 1 + length)
    lo, hi = np.clip(lo[keep], 0, n), np.clip(hi[keep], 0, n)
    ok = hi > lo
    np.add.at(out, lo[ok], 1)
    np.add.at(out, hi[ok], -1)
    return np.cumsum(out)[:n]


def _window_fields(config):
  model = config.window_selector_model
  vr, lin = model.variant_reads_model, model.allele_count_linear_model
  return (int(model.model_type), int(vr.min_num_supporting_reads), int(vr.max_num_supporting_reads),
          int(config.min_allele_support), int(bool(config.enable_strict_insertion_filter)),
          float(lin.bias), float(lin.coeff_soft_clip), float(lin.coeff_substitution), float(lin.coeff_insertion),
          float(lin.coeff_deletion), float(lin.coeff_reference), int(config.min_windows_distance),
          float(lin.decision_boundary))


def _window_key(config, want_debug: bool) -> tuple:
  return _window_fields(config) + (bool(want_debug),)


def _window_options_struct(config, want_debug: bool) -> '_lib.DvWindowOptions':
  return _lib.DvWindowOptions(*_window_fields(config), int(bool(want_debug)), 0)


# ---------------------------------------------------------------- NormalizeCigar (host)
_MATCH_OPS = (1, 8, 9)


def _is_match(op) -> bool:
  return op in _MATCH_OPS


def _merge_operations(cigar: List[List[int]], i: int) -> bool:
  """MergeOperations (:561-590) on cigar[i], cigar[i + 1] = [op, length] pairs."""
  a, b = cigar[i], cigar[i + 1]
  if a[0] == b[0] or (_is_match(a[0]) and _is_match(b[0])):
    a[1] += b[1]
    b[1] = 0
  elif a[0] in (2, 3) and b[0] in (2, 3):
    lo, rest = min(a[1], b[1]), max(a[1], b[1]) - min(a[1], b[1])
    if a[1] > b[1]:
      b[0] = a[0]
    a[0], a[1] = 1, lo
    b[1] = rest
  else:
    return False
  return True


def _swipe_and_merge(cigar: List[List[int]]) -> bool:
  """SwipeAndMerge (:706-730)."""
  modified, merged = False, True
  while merged:
    merged = False
    before = len(cigar)
    cigar[:] = [c for c in cigar if c[1] != 0]
    modified |= len(cigar) < before
    for i in range(len(cigar) - 1):
      if _merge_operations(cigar, i):
        merged = True
        break
    modified |= merged
  return modified


def _handle_heading_indel(cigar: List[List[int]], i: int) -> int:
  """HandleHeadingIndel (:630-648)."""
  if not (i == 0 or (cigar and cigar[0][0] == 5 and i == 1)):
    raise ValueError('Check failed: heading indel position')
  if i >= len(cigar):
    return 0
  if cigar[i][0] == 3:
    shift = cigar[i][1]
    del cigar[i]
    return shift
  if cigar[i][0] == 2:
    shift = -cigar[i][1]
    cigar[i][0] = 1
    return shift
  return 0


def _shift_operation(shift: int, i: int, cigar: List[List[int]]) -> int:
  """ShiftOperation (:654-693)."""
  if i == 0 or (cigar and i == 1 and cigar[0][0] == 5):
    return _handle_heading_indel(cigar, i)
  prev = cigar[i - 1]
  if prev[0] == 5:
    raise ValueError('Check failed: soft clip in the middle of a CIGAR')
  if not _is_match(prev[0]):
    return 0
  if shift > prev[1]:
    raise ValueError('Check failed: shift <= prev_op->operation_length()')
  prev[1] -= shift
  if i + 1 == len(cigar):
    cigar.insert(i + 1, [1, shift])
  else:
    cigar[i + 1][1] += shift
  return 0


def normalize_cigar(read_seq: str, interval_offset: int, cigar: Sequence, ref_bases: str):
  """AlleleCounter::NormalizeCigar (:777-845): left-aligns indels against `ref_bases` (the
  counter's reads-interval reference; `interval_offset` = read start in it).
  -> (is_modified, [CigarUnit], read_shift)."""
  norm = [[c.operation, c.operation_length] for c in cigar]
  read_shift = 0
  if not norm:
    return False, [], 0
  modified = False
  for _ in range(100000000):
    read_offset = 0
    cur = interval_offset + read_shift
    prev_len = norm[0][1]
    shifted = False
    for i, (op, n) in enumerate(norm):
      shift = 0
      if op in (2, 3):
        while prev_len > 0 and (
            (op == 3 and read_offset > 0 and cur + n - 1 < len(ref_bases) and
             read_seq[read_offset - 1] == ref_bases[cur + n - 1]) or
            (op == 2 and cur > 0 and read_offset + n - 1 < len(read_seq) and
             read_seq[read_offset + n - 1] == ref_bases[cur - 1])):
          cur -= 1
          prev_len -= 1
          read_offset -= 1
          shift += 1
        if shift > 0:
          read_shift += _shift_operation(shift, i, norm)
          modified = shifted = True
          break
      prev_len = n
      if op in _MATCH_OPS:
        read_offset += n
        cur += n
      elif op in (5, 2):
        read_offset += n
      elif op in (3, 7, 4):
        cur += n
    merged = _swipe_and_merge(norm)
    modified |= merged
    if not shifted and not merged:
      break
  read_shift += _handle_heading_indel(norm, 0)
  return modified, [T.CigarUnit(op, n) for op, n in norm], read_shift
