"""One region of make_examples, single sample: reads -> window realigner -> allele counts ->
candidate calls -> pileup examples (or, fused, genotype probabilities).  The part of
deepvariant/make_examples_core.py's RegionProcessor that joins the hot path's stages:

  RegionProcessor.realign_reads          make_examples_core.py:2479-2518
  RegionProcessor.candidates_in_region   make_examples_core.py:2840-3165 (one sample; incl. the
                                         two-pass track_ref_reads counting and read phasing with
                                         region padding; gVCF blocks from the device allele counts;
                                         no normalize_reads, no methylation-aware phasing)
  RegionProcessor.process                make_examples_core.py:2215-2380
  partition                              ranges.RangeSet.partition (1000-base calling regions)

Every stage below is this package's own: realigner/ (device allele counts for window
selection, native assembly and alignment), allelecounter.AlleleCounter (device),
variant_calling.VariantCaller (host), direct_phasing.DirectPhasing (native, host),
make_examples_native.ExamplesGenerator (device encoder, optionally fused with the CNN).  With
RegionProcessorOptions.gvcf the regions' gVCF reference blocks come out of the same allele-count
pass (RegionProcessor.gvcf_records; GvcfShardWriter writes them as the reference's gVCF TFRecords).
File handling, sharding, labelling and multi-sample plumbing of the reference's make_examples are
outside SURVEY.md section 8.
"""
from __future__ import annotations

import dataclasses
import os
import numpy as np
from typing import Dict, Iterable, Iterator, List, Optional, Sequence, Tuple

from deepvariant_amd import _lib
from deepvariant_amd import allelecounter
from deepvariant_amd import direct_phasing
from deepvariant_amd import dv_types as T
from deepvariant_amd import make_examples_native
from deepvariant_amd import packing
from deepvariant_amd import sharded_file_utils
from deepvariant_amd import tfrecord
from deepvariant_amd import protowire
from deepvariant_amd import variant_calling
from deepvariant_amd.realigner import realigner as realigner_module
from deepvariant_amd.realigner import utils


@dataclasses.dataclass
class RegionProcessorOptions:
  """The MakeExamplesOptions fields this slice reads (flag defaults of make_examples_options.py)."""
  realigner_enabled: bool = True
  realigner_options: Optional[realigner_module.RealignerOptions] = None    # None = realigner_config()
  realign_on_device: Optional[bool] = None    # the table path's local alignments on the GPU; None = DV_REALIGN_DEVICE
  max_read_length_to_realign: int = 500
  vsc_min_count_snps: int = 2
  vsc_min_count_indels: int = 2
  vsc_min_fraction_snps: float = 0.12
  vsc_min_fraction_indels: float = 0.06
  keep_legacy_allele_counter_behavior: bool = False
  partition_size: int = 1000
  # long-read models (make_examples_options.py:670-700, 1152-1168): phase reads on the fly and
  # tag them HP for the haplotype channel / sort_by_haplotypes; needs track_ref_reads
  track_ref_reads: bool = False
  phase_reads: bool = False
  phase_reads_region_padding_pct: int = 20        # dv_constants.PHASE_READS_REGION_PADDING_PCT
  phase_max_candidates: int = 5000
  min_alleles_to_phase: int = 1
  # --gvcf (make_examples_options.py): reference-confidence blocks of every region, from the allele counts
  gvcf: bool = False
  gvcf_gq_binsize: int = 5
  include_med_dp: bool = False
  # the blocks as arrays only (RegionProcessor.gvcf_block_arrays): gvcf_records stays empty, no Variant per block
  gvcf_arrays_only: bool = False


END_OF_REGION = -1        # make_examples_core.py:125-129: markers in a candidate-positions file
END_OF_PARTITION = -2


class GvcfShardWriter:
  """The gVCF output of one task: serialized nucleus Variant records in a TFRecord file, sharded and
  named as the examples are ('gvcf.tfrecord@N.gz' + task -> 'gvcf.tfrecord-0000t-of-0000N.gz';
  GZIP when the name ends in .gz, tfrecord.Writer's rule).  `with GvcfShardWriter(spec, task) as w:
  w.write_all(records)`."""

  def __init__(self, spec: str, task: int = 0):
    n_shards, self.path = sharded_file_utils.resolve_filespecs(task, spec)
    self.n_shards = n_shards
    self._writer = tfrecord.Writer(self.path)
    self.n_written = 0

  def write(self, variant: T.Variant):
    self._writer.write(protowire.encode_variant(variant))
    self.n_written += 1

  def write_all(self, variants: Iterable[T.Variant]):
    for v in variants:
      self.write(v)

  def close(self):
    self._writer.close()

  def __enter__(self):
    return self

  def __exit__(self, *args):
    self.close()


def partition(region: T.Range, size: int) -> Iterator[T.Range]:
  """Calling regions of at most `size` bases, in order."""
  if size <= 0:
    raise ValueError('partition size must be positive')
  for start in range(region.start, region.end, size):
    yield T.Range(region.reference_name, start, min(start + size, region.end))


def _contig_tuples(contigs) -> List[Tuple[str, int]]:
  return [(c[0], int(c[1])) if isinstance(c, (tuple, list)) else (c.name, int(c.n_bases)) for c in contigs]


def merge_ranges(ranges: Iterable[T.Range], contig_order: Optional[Sequence[str]] = None,
                 known_contigs_only: bool = False) -> List[T.Range]:
  """What iterating a nucleus `RangeSet` yields (third_party/nucleus/util/ranges.py:77-147):
  overlapping AND adjacent ranges merged (`merge_overlaps(strict=False)`), sorted by contig --
  in `contig_order` (the FASTA's) when given, else by name -- then by start.  With
  `known_contigs_only` a range on a contig outside `contig_order` is an error, as it is for a
  RangeSet built with `contigs`."""
  by_contig: Dict[str, List[Tuple[int, int]]] = {}
  for r in ranges:
    by_contig.setdefault(r.reference_name, []).append((int(r.start), int(r.end)))
  if contig_order is not None:
    pos = {name: i for i, name in enumerate(contig_order)}
    if known_contigs_only:
      for name in by_contig:
        if name not in pos:
          raise ValueError('Range on an unrecognized contig: %s' % name)
    names = sorted(by_contig, key=lambda n: (pos.get(n, len(pos)), n))
  else:
    names = sorted(by_contig)
  out = []
  for name in names:
    merged: List[List[int]] = []
    for start, end in sorted(by_contig[name]):
      if merged and start <= merged[-1][1]:          # overlapping or touching
        merged[-1][1] = max(merged[-1][1], end)
      else:
        merged.append([start, end])
    out.extend(T.Range(name, a, b) for a, b in merged)
  return out


def intersect_ranges(a: Sequence[T.Range], b: Sequence[T.Range],
                     contig_order: Optional[Sequence[str]] = None) -> List[T.Range]:
  """`RangeSet.intersection` (ranges.py:204-279): the bases common to both sets; contigs present
  in only one of them drop out."""
  a, b = merge_ranges(a, contig_order), merge_ranges(b, contig_order)
  b_by: Dict[str, List[T.Range]] = {}
  for r in b:
    b_by.setdefault(r.reference_name, []).append(r)
  out = []
  for r in a:
    for o in b_by.get(r.reference_name, ()):
      lo, hi = max(r.start, o.start), min(r.end, o.end)
      if lo < hi:
        out.append(T.Range(r.reference_name, lo, hi))
  return merge_ranges(out, contig_order)


def exclude_ranges(a: Sequence[T.Range], b: Sequence[T.Range],
                   contig_order: Optional[Sequence[str]] = None) -> List[T.Range]:
  """`RangeSet.exclude_regions` (ranges.py:281-300): `a` with every base of `b` chopped out."""
  cut_by: Dict[str, List[T.Range]] = {}
  for r in merge_ranges(b, contig_order):
    cut_by.setdefault(r.reference_name, []).append(r)
  out = []
  for r in merge_ranges(a, contig_order):
    start = r.start
    for c in cut_by.get(r.reference_name, ()):
      if c.end <= start or c.start >= r.end:
        continue
      if c.start > start:
        out.append(T.Range(r.reference_name, start, c.start))
      start = max(start, c.end)
    if start < r.end:
      out.append(T.Range(r.reference_name, start, r.end))
  return out


def build_calling_regions(contigs, regions_to_include: Sequence[T.Range] = (),
                          regions_to_exclude: Sequence[T.Range] = ()) -> List[T.Range]:
  """calling_regions_utils.build_calling_regions (calling_regions_utils.py:48-98) without the
  reference-N exclusion (`--discard_non_dna_regions`, default off): every base of `contigs`,
  intersected with the regions to include if there are any, minus the regions to exclude."""
  contigs = _contig_tuples(contigs)
  order = [name for name, _ in contigs]
  regions = [T.Range(name, 0, n) for name, n in contigs]
  if regions_to_include:
    regions = intersect_ranges(regions, regions_to_include, order)
  if regions_to_exclude:
    regions = exclude_ranges(regions, regions_to_exclude, order)
  return merge_ranges(regions, order)


def regions_to_process(contigs, partition_size: int, calling_regions: Optional[Sequence[T.Range]] = None,
                       task_id: Optional[int] = None, num_shards: Optional[int] = None,
                       round_robin_sampling: bool = True) -> List[T.Range]:
  """make_examples_core.regions_to_process (make_examples_core.py:800-888): the contigs'
  bases (intersected with `calling_regions`), in FASTA contig order, cut into pieces of at
  most `partition_size`; with shards, task `task_id` takes the pieces i % num_shards ==
  task_id -- the rule the reference applies whenever examples go to TFRecords, and the rule
  the ranks of a multi-GPU run use (deepvariant_amd/dist.py) -- or, without round robin, the
  task_id-th block of ceil(n / num_shards) consecutive pieces."""
  if (task_id is None) != (num_shards is None):
    raise ValueError('Both task_id and num_shards must be present if either is', task_id, num_shards)
  if num_shards:
    if num_shards < 0:
      raise ValueError('num_shards={} must be >= 0'.format(num_shards))
    if task_id < 0 or task_id >= num_shards:
      raise ValueError('task_id={} should be >= 0 and < num_shards={}'.format(task_id, num_shards))
  contigs = _contig_tuples(contigs)
  order = [name for name, _ in contigs]
  regions = [T.Range(name, 0, n) for name, n in contigs]
  if calling_regions:
    regions = intersect_ranges(regions, calling_regions, order)
  else:
    regions = merge_ranges(regions, order)
  pieces = [p for r in regions for p in partition(r, partition_size)]
  if num_shards:
    if round_robin_sampling:
      return [p for i, p in enumerate(pieces) if i % num_shards == task_id]
    per_shard = -(-len(pieces) // num_shards)
    return pieces[task_id * per_shard:(task_id + 1) * per_shard]
  return pieces


@dataclasses.dataclass
class VcfSink:
  """What flush_queue needs to turn the classifier's output into finished VCF records, and where they collect."""
  qual_filter: float = 1.0
  cnn_homref_call_min_gq: float = 20.0
  sample_name: Optional[str] = None
  want_records: bool = True                  # CallVariantsOutput records beside the VCF
  n_examples: int = 0                        # classified so far
  records: List = dataclasses.field(default_factory=list)
  device_stats: Dict[str, int] = dataclasses.field(default_factory=dict)    # dv_genotype_device_stats, summed


class RegionProcessor:
  def __init__(self, options: T.MakeExamplesOptions, ref_reader, processor_options: Optional[RegionProcessorOptions] = None,
               example_filenames: Optional[Dict[str, str]] = None, device: int = 0):
    if len(options.sample_options) != 1:
      raise NotImplementedError('RegionProcessor handles one sample; multi-sample regions go through '
                                'ExamplesGenerator directly')
    self.options = options
    self.ref_reader = ref_reader
    self.processor_options = processor_options or RegionProcessorOptions()
    po = self.processor_options
    if po.phase_reads and not po.track_ref_reads:
      raise ValueError('--track_ref_reads must be set to True when --phase_reads is set.')
    self.direct_phasing = direct_phasing.DirectPhasing(po.min_alleles_to_phase) if po.phase_reads else None
    self.realigner = None
    if po.realigner_enabled:
      self.realigner = realigner_module.Realigner(po.realigner_options or realigner_module.realigner_config(),
                                                  ref_reader, device_align=po.realign_on_device)
    sample = options.sample_options[0]
    self.variant_caller = variant_calling.VariantCaller(variant_calling.VariantCallerOptions(
        po.vsc_min_count_snps, po.vsc_min_count_indels, po.vsc_min_fraction_snps, po.vsc_min_fraction_indels,
        sample_name=sample.name, track_ref_reads=po.track_ref_reads, gq_resolution=po.gvcf_gq_binsize))
    # with po.gvcf: the gVCF records of the regions of the last process / process_table(s) call, one list
    # per region in call order (empty for a region without reads, as in the reference)
    self.gvcf_records: List[List[T.Variant]] = []
    # the same blocks as allelecounter.GVCF_BLOCK_DTYPE arrays, one per region in call order
    self.gvcf_block_arrays: List[np.ndarray] = []
    self._queue: List = []
    self.n_queued_examples = 0
    self.vcf: Optional[VcfSink] = None       # --vcf_outfile: flush_queue merges each site's calls and collects the records
    self.generator = make_examples_native.ExamplesGenerator(
        options, example_filenames or {}, test_mode=not example_filenames, device=device, ref_reader=ref_reader)

  def realign_reads(self, reads: Sequence, region: T.Range) -> List:
    """Reads longer than max_read_length_to_realign bypass the realigner and come first."""
    if self.realigner is None:
      return list(reads)
    limit = self.processor_options.max_read_length_to_realign
    if limit == 0:
      return self.realigner.realign_reads(reads, region)[1]
    long_reads = [r for r in reads if len(r.aligned_sequence) > limit]
    short_reads = [r for r in reads if len(r.aligned_sequence) <= limit]
    return long_reads + self.realigner.realign_reads(short_reads, region)[1]

  def _allele_counter(self, region: T.Range, table, candidate_positions=()):
    rr = self.options.pic_options.read_requirements
    counter = allelecounter.AlleleCounter(
        self.ref_reader, region.reference_name, region.start, region.end,
        candidate_positions=candidate_positions, min_mapping_quality=rr.min_mapping_quality,
        min_base_quality=rr.min_base_quality,
        keep_legacy_behavior=self.processor_options.keep_legacy_allele_counter_behavior,
        track_ref_reads=self.processor_options.track_ref_reads)
    counter.add_table(table)        # the region's reads are packed once for both passes
    return counter

  def candidates_in_region(self, region: T.Range, reads: Sequence,
                           padded_region: Optional[T.Range] = None) -> List[T.DeepVariantCall]:
    """Allele counts over the (padded) region from the reads that overlap `region` (one kernel
    launch; two with track_ref_reads: the first finds the positions that will be called, the
    second keeps their reference-supporting reads by name), the candidate caller, and -- with
    phase_reads -- the phasing of those reads (their HP tags are REPLACED in place)."""
    po = self.processor_options
    in_region = [r for r in reads if utils.ranges_overlap(utils.read_range(r), region)]
    self.gvcf_records = [[]] if po.gvcf else []
    self.gvcf_block_arrays = [np.zeros(0, allelecounter.GVCF_BLOCK_DTYPE)] if po.gvcf else []
    if not in_region:
      return []
    effective = padded_region or region
    table = packing.ReadTable.from_reads(in_region)
    positions = ()
    if po.track_ref_reads:
      first_pass = self._allele_counter(effective, table)
      positions = self.variant_caller.call_positions_from_allele_counter(first_pass)
    counter = self._allele_counter(effective, table, positions)
    if po.gvcf:
      # summary_counts(left_padding, right_padding): the padding of a padded region is not reported
      opts = self._gvcf_options(region.start - effective.start, effective.end - region.end)
      allelecounter.AlleleCounter.run_batch([counter], gvcf=opts, **self._device_call())
      self._keep_gvcf(0, counter, opts)
    candidates = self.variant_caller.calls_from_allele_counter(counter)
    if self.direct_phasing is not None:
      to_phase = [r for r in in_region if utils.ranges_overlap(utils.read_range(r), effective)]
      for read in to_phase:
        read.info.pop('HP', None)                 # an existing phasing must not leak into the images
      if not (po.phase_max_candidates and len(candidates) > po.phase_max_candidates):
        for read, phase in zip(to_phase, self.direct_phasing.phase(candidates, to_phase)):
          if self.options.pic_options.reverse_haplotypes and phase in (1, 2):
            phase = 1 + (phase % 2)
          read.info['HP'] = T.ListValue(values=[T.Value(int_value=int(phase))])
    if padded_region is not None:                 # filter_candidates_by_region, :2579-2606
      candidates = [c for c in candidates if region.start <= c.variant.start < region.end]
    return candidates

  def _device_call(self, positions_only: bool = False) -> dict:
    """run_batch's `call=` argument when the counter offers the device candidate caller (candidates.hip):
    the candidates then come out of the counting pass; {} otherwise (the caller walks the counts)."""
    if getattr(allelecounter.AlleleCounter, 'candidates', None) is None:
      return {}
    return {'call': self.variant_caller.candidate_options(positions_only)}

  def _keep_gvcf(self, k: int, counter, opts) -> None:
    """Region k's blocks from its counter: the array, and the Variant records unless gvcf_arrays_only."""
    self.gvcf_block_arrays[k] = counter.gvcf_block_array(opts)
    if not self.processor_options.gvcf_arrays_only:
      self.gvcf_records[k] = counter.gvcf_blocks(opts)

  def _gvcf_options(self, left_padding: int = 0, right_padding: int = 0) -> 'variant_calling.GvcfOptions':
    caller_options = self.variant_caller._options          # pylint: disable=protected-access
    return variant_calling.GvcfOptions.from_caller_options(caller_options, self.processor_options.include_med_dp,
                                                           left_padding, right_padding)

  def find_candidate_positions(self, region: T.Range, reads: Sequence) -> List[int]:
    """candidate_sweep mode (make_examples_core.py:2117-2189): the positions at which the RAW reads
    of the region (no realigner) would make the caller emit a candidate, then END_OF_PARTITION."""
    in_region = [r for r in reads if utils.ranges_overlap(utils.read_range(r), region)]
    if not in_region:
      return [END_OF_PARTITION]
    counter = self._allele_counter(region, packing.ReadTable.from_reads(in_region))
    return self.variant_caller.call_positions_from_allele_counter(counter) + [END_OF_PARTITION]

  def process(self, region: T.Range, reads: Sequence) -> Tuple[List[T.DeepVariantCall], List]:
    """-> (candidates, the region's reads as the pileup images must see them)."""
    po = self.processor_options
    realigned = self.realign_reads(reads, region)
    padded = None
    if po.phase_reads:
      # HP tags are written on this region's own copies: a long read that overlaps two calling
      # regions is phased in each (the labels 1 / 2 are only meaningful within a region)
      realigned = [dataclasses.replace(r, info=dict(r.info)) for r in realigned]
      if po.phase_reads_region_padding_pct > 0:
        padding = int((region.end - region.start) * po.phase_reads_region_padding_pct / 100)
        padded = utils.expand(region, padding, self.ref_reader.n_bases(region.reference_name))
    return self.candidates_in_region(region, realigned, padded), realigned

  # ---- the table path: the region's reads stay a packed table from the BAM decoder to the
  # encoder (make_examples.RegionReads.table); no Read objects.  It covers the default short-read
  # calling configuration, window-trimmed pileups (trim_reads_for_pileup /
  # keep_only_window_spanning_reads: alt_aligned_pileup_lib.trim_table) and, behind
  # DV_PHASE_TABLES=1 (read at each call, as DV_REALIGN_DEVICE is), read phasing (phase_reads:
  # _phase_tables below) and, behind DV_ALT_ALIGN_TABLES=1 (read at each call too), alt-aligned
  # pileups (alt_aligned_pileup_lib.alt_align_table realigns the trimmed table to the alt
  # haplotypes); everything that works on Read objects (spliced-read splitting, channels with
  # per-read aux pixels) takes the object path above.
  def table_path_ok(self) -> bool:
    import os
    from deepvariant_amd import alt_aligned_pileup_lib as aap
    po, gen = self.processor_options, self.generator
    return ((not po.phase_reads or os.environ.get('DV_PHASE_TABLES') == '1') and
            not (self.realigner is not None and self.realigner.config.split_skip_reads) and
            (gen._alt_mode == aap.NONE or os.environ.get('DV_ALT_ALIGN_TABLES') == '1') and   # pylint: disable=protected-access
            not gen._encoder_api._need_aux and not gen._encoder_api._need_seq_aux)   # pylint: disable=protected-access

  def realign_table(self, table, region: T.Range):
    """realign_reads on a table: reads longer than max_read_length_to_realign bypass the
    realigner and come first."""
    return self.realign_tables([table], [region])[0]

  def realign_tables(self, tables: Sequence, regions: Sequence[T.Range]) -> List:
    """`realign_table` for a batch of calling regions: the realigner's assembly and alignment
    work of all of them goes through one native, threaded call (Realigner.realign_tables)."""
    return self.start_realign_tables(tables, regions)()

  def start_realign_tables(self, tables: Sequence, regions: Sequence[T.Range], executor=None):
    """-> a callable that returns the realigned tables.  The regions' windows are selected now;
    with an `executor` the native call is already running on one of its threads when this
    returns (Realigner.start_realign_tables)."""
    tables = list(tables)
    if self.realigner is None:
      return lambda: tables
    limit = self.processor_options.max_read_length_to_realign
    long_parts = [None] * len(tables)
    short = tables
    if limit:
      short = []
      for k, table in enumerate(tables):
        lengths = np.diff(table.read_seq_off.astype(np.int64))
        long_rows = np.nonzero(lengths > limit)[0]
        if len(long_rows):
          long_parts[k] = table.take(long_rows)
          table = table.take(np.nonzero(lengths <= limit)[0])
        short.append(table)
    job = self.realigner.start_realign_tables(short, regions, want_haplotypes=False, executor=executor)

    def finish():
      return [t if lp is None else packing.concat_tables([lp, t])
              for lp, (_, t) in zip(long_parts, job.result())]
    return finish

  def process_table(self, region: T.Range, table, realigned=None) -> Tuple[List[T.DeepVariantCall], 'packing.ReadTable']:
    """`realigned`: the region's table as `realign_tables` returned it (the runner realigns a
    batch of regions ahead); None = realign here."""
    return self.process_tables([region], [table], None if realigned is None else [realigned])[0]

  def process_tables(self, regions: Sequence[T.Range], tables: Sequence, realigned_tables: Optional[Sequence] = None
                     ) -> List[Tuple[List[T.DeepVariantCall], 'packing.ReadTable']]:
    """Candidates of a batch of calling regions: -> [(candidates, realigned table)] per region.  The
    regions' allele counters are filled in one device call per pass (AlleleCounter.run_batch: one
    upload, kernels back to back -- two passes with track_ref_reads, the first of which brings home
    the candidate positions only), and the candidate caller runs behind the counter on the device
    (AlleleCounter.candidates); the calls are then built region by region for its sites."""
    if realigned_tables is None:
      realigned_tables = self.realign_tables(tables, regions)
    po = self.processor_options
    # with phase_reads the counters run over the padded region, as `process` does
    effective = list(regions)
    if po.phase_reads and po.phase_reads_region_padding_pct > 0:
      effective = [utils.expand(r, int((r.end - r.start) * po.phase_reads_region_padding_pct / 100),
                                self.ref_reader.n_bases(r.reference_name)) for r in regions]
    out = [([], realigned) for realigned in realigned_tables]
    slots, in_region, rows_of = [], [], []
    for k, (region, realigned) in enumerate(zip(regions, realigned_tables)):
      rows = np.nonzero((realigned.read_end > region.start) & (region.end > realigned.read_pos.astype(np.int64)))[0]
      if len(rows):
        slots.append(k)
        in_region.append(realigned.take(rows))
        rows_of.append(rows)
    run_batch = getattr(allelecounter.AlleleCounter, 'run_batch', None) or (lambda counters, **kwargs: None)
    positions = [()] * len(slots)
    if po.track_ref_reads:
      first_pass = [self._allele_counter(effective[k], t) for k, t in zip(slots, in_region)]
      run_batch(first_pass, **self._device_call(positions_only=True))
      positions = [self.variant_caller.call_positions_from_allele_counter(c) for c in first_pass]
    counters = [self._allele_counter(effective[k], t, p) for k, t, p in zip(slots, in_region, positions)]
    if po.gvcf:
      # the same counts, with the regions' gVCF blocks computed behind them on the device
      self.gvcf_records = [[] for _ in regions]
      self.gvcf_block_arrays = [np.zeros(0, allelecounter.GVCF_BLOCK_DTYPE) for _ in regions]
      if po.phase_reads:
        # summary_counts(left_padding, right_padding): the padding of a padded region is not reported
        for k, counter in zip(slots, counters):
          opts = self._gvcf_options(regions[k].start - effective[k].start, effective[k].end - regions[k].end)
          allelecounter.AlleleCounter.run_batch([counter], gvcf=opts, **self._device_call())
          self._keep_gvcf(k, counter, opts)
      else:
        opts = self._gvcf_options()
        allelecounter.AlleleCounter.run_batch(counters, gvcf=opts, **self._device_call())
        for k, counter in zip(slots, counters):
          self._keep_gvcf(k, counter, opts)
    else:
      run_batch(counters, **self._device_call())
    phased = self._phase_tables(slots, counters, in_region, rows_of, realigned_tables) if po.phase_reads else {}
    for k, counter, rows in zip(slots, counters, rows_of):
      candidates = self.variant_caller.calls_from_allele_counter(counter)
      if effective[k] is not regions[k]:              # filter_candidates_by_region
        candidates = [c for c in candidates if regions[k].start <= c.variant.start < regions[k].end]
      for c in candidates:
        # the caller's rows are those of the counter's table (the region's rows of the realigned one): as rows of
        # the table the region is packed from
        if c.support_rows is not None:
          c.support_rows = {allele: rows[r] for allele, r in c.support_rows.items()}
      out[k] = (candidates, phased.get(k, realigned_tables[k]))
    return out

  def _phase_tables(self, slots, counters, in_region, rows_of, realigned_tables) -> Dict[int, 'packing.ReadTable']:
    """Read phasing on tables: the regions' phasing arrays straight from their counters' events
    (AlleleCounter.phasing_arrays), ONE device call for the batch (direct_phasing.phase_arrays), and the phases
    written into a copy of each region's table's read_hp for the rows that overlap the region -- the reads
    `candidates_in_region` phases.  Rows it leaves alone keep their read_hp.  -> {slot: table}."""
    po = self.processor_options
    call = self.variant_caller.candidate_options()
    arrays, which, tables = [], [], {}
    for k, counter, table, rows in zip(slots, counters, in_region, rows_of):
      parts = counter.phasing_arrays(call)
      hp = realigned_tables[k].read_hp.copy()
      hp[rows] = _lib.DV_HP_NONE                      # an existing phasing must not leak into the images
      tables[k] = dataclasses.replace(realigned_tables[k], read_hp=hp)
      if not (po.phase_max_candidates and len(parts[0]) > po.phase_max_candidates):
        arrays.append(parts + (table.n_reads,))
        which.append((hp, rows))
    if arrays:
      results = direct_phasing.phase_arrays(arrays, po.min_alleles_to_phase, device=True)
      for (hp, rows), (phases, _, _) in zip(which, results):
        if self.options.pic_options.reverse_haplotypes:
          phases = np.where(phases > 0, 3 - phases, phases)
        hp[rows] = phases
    return tables

  def examples_in_region_table(self, region: T.Range, table, stats: Optional[dict] = None, realigned=None,
                               called=None) -> Tuple[List[T.DeepVariantCall], List[bytes]]:
    """`called`: (candidates, realigned table) of this region out of `process_tables`."""
    candidates, realigned = called if called is not None else self.process_table(region, table, realigned)
    if not candidates:
      return candidates, []
    examples, _ = self.generator.encode_region(candidates, [realigned], [0], [0.0], stats if stats is not None else {})
    return candidates, examples

  def call_variants_in_region_table(self, region: T.Range, table, model) -> Tuple[List[T.DeepVariantCall], List[bytes]]:
    candidates, realigned = self.process_table(region, table)
    if not candidates:
      return candidates, []
    return candidates, self.generator.call_variants_in_region(candidates, [realigned], [0], [0.0], model)

  # ---- deferred classification (table path, fused route): regions are drawn on the device one by
  # one, their tensors wait there, and ONE CNN forward classifies a few hundred examples
  def queue_region_table(self, region: T.Range, table, model, realigned=None) -> List[T.DeepVariantCall]:
    candidates, realigned = self.process_table(region, table, realigned)
    return self.queue_region_candidates(candidates, realigned, model)

  def queue_region_candidates(self, candidates, realigned, model) -> List[T.DeepVariantCall]:
    """The drawing half of queue_region_table, for a driver that called the candidates of a batch
    of regions at once (process_tables)."""
    images, plan = (None, [])
    if candidates:
      images, plan = self.generator.encode_region_on_device(candidates, [realigned], [0], [0.0], model.input_shape)
    self._queue.append((candidates, plan, images))
    self.n_queued_examples += len(plan)
    return candidates

  def queue_regions_candidates(self, called, model) -> None:
    """queue_region_candidates for a batch of regions (`called`: process_tables' [(candidates, realigned table)]):
    the regions that qualify are packed on the device by one call and drawn by one encoder launch
    (ExamplesGenerator.encode_regions_on_device, DV_PACK_DEVICE=1); the others take the per-region call.  The
    queue gets the same (candidates, plan, images) entries, in region order."""
    gen = self.generator
    batched = [k for k, (candidates, realigned) in enumerate(called) if candidates and gen.device_pack_ok(realigned)]
    drawn = {}
    if batched:
      results = gen.encode_regions_on_device([called[k] for k in batched], model.input_shape)
      drawn = dict(zip(batched, results))
    for k, (candidates, realigned) in enumerate(called):
      if k in drawn:
        images, plan = drawn[k]
        self._queue.append((candidates, plan, images))
        self.n_queued_examples += len(plan)
      else:
        self.queue_region_candidates(candidates, realigned, model)

  def flush_queue(self, model) -> List[List[bytes]]:
    """-> the CallVariantsOutput records of every queued region, in queue order.  Examples are
    classified independently of their batch (no kernel reduces across examples), so the records
    are the ones region-by-region classification gives, byte for byte."""
    import torch
    from deepvariant_amd import call_variants as cv
    queue, self._queue, self.n_queued_examples = self._queue, [], 0
    tensors = [img for _, plan, img in queue if plan]
    out: List[List[bytes]] = []
    if not tensors:
      return [[] for _ in queue]
    limit = model.max_batch
    stacked = torch.cat(tensors) if len(tensors) > 1 else tensors[0]
    if self.vcf is not None:
      probs = [model(stacked[i:i + limit]) for i in range(0, stacked.shape[0], limit)]
      gls = self._genotype_queue(queue, torch.cat(probs) if len(probs) > 1 else probs[0])
      if not self.vcf.want_records:
        return [[] for _ in queue]
    else:
      rows = [cv.round_gls_batch(model(stacked[i:i + limit]).cpu().numpy(), 10) for i in range(0, stacked.shape[0], limit)]
      gls = np.concatenate(rows)
    at = 0
    for candidates, plan, _ in queue:
      out.append(self.generator.call_variants_outputs(candidates, plan, gls[at:at + len(plan)]) if plan else [])
      at += len(plan)
    return out

  @staticmethod
  def queue_sites(queue):
    """The queue's plans as sites: -> ([the variant of each site], postprocess_variants.site_tables of them).  A site
    is one candidate, its items the plan's examples of it, which follow each other."""
    from deepvariant_amd import postprocess_variants as pp
    variants, sites = [], []
    for candidates, plan, _ in queue:
      last = None
      for ci, combo in plan:
        variant = candidates[ci].variant
        if ci != last:
          variants.append(variant)
          sites.append((len(variant.alternate_bases), []))
          last = ci
        sites[-1][1].append(sorted(make_examples_native.encode_alt_alleles(variant, combo)[1]))
    return variants, pp.site_tables(sites)

  def _genotype_queue(self, queue, probs) -> np.ndarray:
    """--vcf_outfile: the queue's sites merged on the device from the classifier's output tensor where it lies
    (postprocess_variants.genotype_sites_device; DV_GENOTYPE_HOST=1: downloaded and merged by the host code), their
    finished records added to self.vcf.records.  A site is one candidate, its items the plan's examples of it.
    -> the rounded likelihood rows, float64 [N, 3], what round_gls_batch gives."""
    from deepvariant_amd import postprocess_variants as pp
    variants, tables = self.queue_sites(queue)
    vcf = self.vcf
    vcf.n_examples += int(probs.shape[0])
    if os.environ.get('DV_GENOTYPE_HOST', '0') not in ('', '0'):
      result = pp.genotype_sites(probs.cpu().numpy(), *tables, qual_filter=vcf.qual_filter)
    else:
      result = pp.genotype_sites_device(probs.contiguous(), *tables, qual_filter=vcf.qual_filter)
      stats = pp.last_device_stats()
      for name, value in stats.items():
        vcf.device_stats[name] = vcf.device_stats.get(name, 0) + value
    pp.check_status(result, lambda i: probs[i].cpu().numpy(), tables[1], lambda s: pp.describe_variant(variants[s]))
    vcf.records.extend(pp.finish_sites(variants, result, vcf.qual_filter, vcf.cnn_homref_call_min_gq, vcf.sample_name))
    return result.rounded

  def examples_in_region(self, region: T.Range, reads: Sequence, stats: Optional[dict] = None
                         ) -> Tuple[List[T.DeepVariantCall], List[bytes]]:
    """-> (candidates, serialised tf.Examples in candidate / alt-combination order)."""
    candidates, realigned = self.process(region, reads)
    if not candidates:
      return candidates, []
    examples, _ = self.generator.encode_region(candidates, [realigned], [0], [0.0], stats if stats is not None else {})
    return candidates, examples

  def call_variants_in_region(self, region: T.Range, reads: Sequence, model) -> Tuple[List[T.DeepVariantCall], List[bytes]]:
    """Fused: -> (candidates, serialised CallVariantsOutput per example); the images never
    leave the device."""
    candidates, realigned = self.process(region, reads)
    if not candidates:
      return candidates, []
    return candidates, self.generator.call_variants_in_region(candidates, [realigned], [0], [0.0], model)
