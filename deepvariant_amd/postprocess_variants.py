"""MI355X `postprocess_variants`: CallVariantsOutput records -> one genotype, GQ and QUAL per site -> VCF.

This project's restatement of the reference's `deepvariant/postprocess_variants.py` (`merge_predictions`,
`get_alt_alleles_to_remove`, `convert_call_variants_outputs_to_probs_dict`, `add_call_to_variant`, `compute_quals`)
and nucleus `genomics_math.py`; DESIGN.md section 21 is the contract and lists what is remembered, not pinned.

Steps 1 to 3 (rounding, which alts to drop, the merge) are native: `genotype_sites` is the host code
(dv_genotype_sites), `genotype_sites_device` the kernel (dv_genotype_sites_device, csrc/genotype.hip), which reads the
classifier's output tensor where it lies.  Both return the same arrays bit for bit.  Step 4 (`finish_sites`: phred
scores, the call, pruned and simplified alleles) needs log10 and is one host function for both routes.

The gVCF: `merge_blocks_and_variants` (dv_gvcf_merge) and `merge_blocks_and_variants_device`
(dv_gvcf_merge_device, csrc/gvcf_merge.hip) interleave the reference blocks of the allele counter with the finished
records -- both return the same arrays -- and `gvcf_text` / `write_gvcf` print the rows; with rows='native'
(DV_GVCF_ROWS_NATIVE=1) `gvcf_body_native` merges and prints in one native call (section 23, csrc/gvcf_rows.hip).
Blocks travel as `allelecounter.GVCF_BLOCK_DTYPE` arrays per contig from end to end; no object is made per block.
With DV_BGZF=1 a name that ends in .gz is written as BGZF: `bgzf_compress` is the host code
(dv_bgzf_compress) or, with `device`, the kernels of csrc/bgzf.hip; with the native rows as well `gvcf_file_native`
takes the whole .g.vcf.gz from one call (dv_gvcf_rows_bgzf[_device]), deflated on the device where the rows were written.

  python -m deepvariant_amd.postprocess_variants --infile CVO --ref FASTA --outfile VCF
      [--nonvariant_site_tfrecord_path GVCF_TFRECORDS --gvcf_outfile GVCF]
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import gzip
import math
import os
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np

from deepvariant_amd import _lib
from deepvariant_amd import dv_types as T

_MAX_CONFIDENCE = 1.0 - 1e-15            # genomics_math.ptrue_to_bounded_phred's max_prob
DEFAULT_QUAL_FILTER = 1.0                # --qual_filter
DEFAULT_CNN_HOMREF_CALL_MIN_GQ = 20.0    # --cnn_homref_call_min_gq
OK, BAD_SUM, INCOMPLETE = _lib.DV_GENOTYPE_OK, _lib.DV_GENOTYPE_BAD_SUM, _lib.DV_GENOTYPE_INCOMPLETE


# ------------------------------------------------------------------------------------------ steps 1 to 3, native
@dataclasses.dataclass
class SiteGenotypes:
  """One call's arrays (dv_genotypes_view, copied)."""
  rounded: np.ndarray        # float64 [N, 3]
  pred_off: np.ndarray       # int64 [S + 1]
  predictions: np.ndarray    # float64; site s owns [pred_off[s], pred_off[s + 1]), the kept alleles' genotypes first
  best: np.ndarray           # int32 [S]
  removed: np.ndarray        # uint32 [S], a bit per removed alt
  status: np.ndarray         # uint8 [S]

  def n_kept_alts(self, site: int) -> int:
    slots = int(self.pred_off[site + 1] - self.pred_off[site])
    alts = (math.isqrt(8 * slots + 1) - 3) // 2
    return alts - bin(int(self.removed[site])).count('1')

  def site_predictions(self, site: int) -> List[float]:
    kept = self.n_kept_alts(site)
    at = int(self.pred_off[site])
    return self.predictions[at:at + (kept + 1) * (kept + 2) // 2].tolist()


def min_nonref_prob(qual_filter: float) -> float:
  """Step 2's threshold: the smallest probability whose QUAL reaches `qual_filter` (dv_genotype_min_nonref_prob)."""
  return float(_lib.lib().dv_genotype_min_nonref_prob(float(qual_filter)))


def _tables(item_alts, site_off, n_alts):
  alts = np.ascontiguousarray(item_alts, np.int8).reshape(-1, 2)
  off = np.ascontiguousarray(site_off, np.int32).reshape(-1)
  n = np.ascontiguousarray(n_alts, np.int32).reshape(-1)
  if off.size != n.size + 1:
    raise ValueError('site_off must have one entry more than n_alts')
  return alts, off, n


def _take(handle) -> SiteGenotypes:
  l = _lib.lib()
  try:
    view = _lib.DvGenotypesView()
    _lib.check(l.dv_genotypes_arrays(handle, C.byref(view)))

    def array(ptr, count, dtype):
      if count == 0:
        return np.zeros(0, dtype)
      return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint8)),
                                   (count * np.dtype(dtype).itemsize,)).view(dtype).copy()
    s = view.n_sites
    return SiteGenotypes(rounded=array(view.rounded, view.n_items * 3, np.float64).reshape(-1, 3),
                         pred_off=array(view.pred_off, s + 1, np.int64),
                         predictions=array(view.predictions, view.n_predictions, np.float64),
                         best=array(view.best, s, np.int32), removed=array(view.removed, s, np.uint32),
                         status=array(view.status, s, np.uint8))
  finally:
    l.dv_genotypes_free(handle)


def genotype_sites(probs, item_alts, site_off, n_alts, qual_filter: float = DEFAULT_QUAL_FILTER,
                   t: Optional[float] = None, already_rounded: bool = False) -> SiteGenotypes:
  """The host code.  probs float32 [N, 3]; item_alts int8 [N, 2] (the second -1 for one alt); site_off int32
  [S + 1]; n_alts int32 [S].  `t` overrides min_nonref_prob(qual_filter).  already_rounded: the rows are the rounded
  values of CallVariantsOutput records and are not rounded again (round_gls is not idempotent in float32)."""
  p = np.ascontiguousarray(probs, np.float32).reshape(-1, 3)
  alts, off, n = _tables(item_alts, site_off, n_alts)
  if alts.shape[0] != p.shape[0]:
    raise ValueError('one item_alts row per probability row is expected')
  handle = C.c_void_p()
  _lib.check(_lib.lib().dv_genotype_sites(p.ctypes.data, p.shape[0], alts.ctypes.data, n.size, off.ctypes.data,
                                          n.ctypes.data, min_nonref_prob(qual_filter) if t is None else float(t),
                                          1 if already_rounded else 0, C.byref(handle)))
  return _take(handle)


def genotype_sites_device(probs, item_alts, site_off, n_alts, qual_filter: float = DEFAULT_QUAL_FILTER,
                          stream=None, t: Optional[float] = None) -> SiteGenotypes:
  """The same on the device.  `probs` is a float32 [N, 3] NumPy array (staged and uploaded) or a contiguous CUDA
  tensor, read in place: on the tensor's current stream, or -- when that is the default stream -- after waiting for
  it, on a stream the library owns.  `stream` (a raw handle) overrides; `t` as in genotype_sites."""
  alts, off, n = _tables(item_alts, site_off, n_alts)
  if isinstance(probs, np.ndarray):
    p = np.ascontiguousarray(probs, np.float32).reshape(-1, 3)
    pointer, memory, rows = p.ctypes.data, _lib.DV_MEM_HOST, p.shape[0]
  else:
    import torch  # device memory + stream only
    p = probs
    if not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous() or p.dim() != 2 or p.shape[1] != 3:
      raise ValueError('a contiguous float32 [N, 3] CUDA tensor is expected')
    pointer, memory, rows = p.data_ptr(), _lib.DV_MEM_DEVICE, p.shape[0]
    if stream is None:
      current = torch.cuda.current_stream(p.device)
      stream = current.cuda_stream
      if not stream:
        current.synchronize()
  if alts.shape[0] != rows:
    raise ValueError('one item_alts row per probability row is expected')
  handle = C.c_void_p()
  _lib.check(_lib.lib().dv_genotype_sites_device(pointer, memory, rows, alts.ctypes.data, n.size, off.ctypes.data,
                                                 n.ctypes.data, min_nonref_prob(qual_filter) if t is None else float(t),
                                                 C.byref(handle), C.c_void_p(stream or None)))
  return _take(handle)


def last_device_stats() -> Dict[str, int]:
  stats = _lib.DvGenotypeDeviceStats()
  _lib.check(_lib.lib().dv_genotype_device_last_stats(C.byref(stats)))
  return {name: int(getattr(stats, name)) for name, _ in stats._fields_}


def site_tables(sites: Sequence[Tuple[int, Sequence[Sequence[int]]]]):
  """[(n_alts, [the alt indices of each item])] -> (item_alts, site_off, n_alts)."""
  item_alts, site_off, n_alts = [], [0], []
  for alts, items in sites:
    for indices in items:
      indices = list(indices)
      if not 1 <= len(indices) <= 2:
        raise ValueError('an item names one or two alts, got %s' % (indices,))
      item_alts.append((indices[0], indices[1] if len(indices) == 2 else -1))
    site_off.append(len(item_alts))
    n_alts.append(alts)
  return (np.array(item_alts, np.int8).reshape(-1, 2), np.array(site_off, np.int32), np.array(n_alts, np.int32))


def check_status(result: SiteGenotypes, probs_row, site_off, describe) -> None:
  """BAD_SUM raises round_gls' ValueError, INCOMPLETE a ValueError naming the site.  probs_row(i) -> item i's
  float32 probabilities; describe(s) -> text for site s."""
  bad = np.nonzero(result.status != OK)[0]
  if not bad.size:
    return
  site = int(bad[0])
  if result.status[site] == BAD_SUM:
    for i in range(int(site_off[site]), int(site_off[site + 1])):
      row = np.asarray(probs_row(i), np.float32)
      total = (row[0] + row[1]) + row[2]
      if np.abs(total - np.float32(1)) > np.float32(1e-6):
        raise ValueError('Invalid genotype likelihoods do not sum to one: sum({}) = {}'.format(list(row), total))
  raise ValueError('%s: its examples do not cover every genotype of its alleles' % describe(site))


# ------------------------------------------------------------------------------------------ step 4, host
def _phred(p: float) -> float:
  """genomics_math.ptrue_to_bounded_phred."""
  return -10.0 * math.log10(1.0 - min(p, _MAX_CONFIDENCE))


def compute_quals(predictions: Sequence[float], prediction_index: int) -> Tuple[int, float]:
  """-> (GQ, QUAL): the phred of the called genotype, and of any non-reference genotype."""
  gq = int(np.around(_phred(predictions[prediction_index])))
  qual = round(_phred(min(sum(predictions[1:]), 1.0)), 7)
  return gq, qual


def most_likely_genotype(predictions: Sequence[float]) -> Tuple[int, List[int]]:
  """-> (the first index of the largest prediction, its diploid genotype in VCF order)."""
  index = max(range(len(predictions)), key=predictions.__getitem__)
  return index, genotype_of_index(index)


def genotype_of_index(index: int) -> List[int]:
  b = (math.isqrt(8 * index + 1) - 1) // 2
  return [index - b * (b + 1) // 2, b]


def _call_values(variant: T.Variant, key: str) -> Optional[list]:
  if not variant.calls or key not in variant.calls[0].info:
    return None
  out = []
  for v in variant.calls[0].info[key].values:
    out.append(v.int_value if v.int_value is not None else v.number_value)
  return out


def prune_alleles(variant: T.Variant, removed: int):
  """-> (alts, AD, VAF) without the alts whose bit is set in `removed`; AD keeps its leading reference entry."""
  keep = [a for a in range(len(variant.alternate_bases)) if not (removed >> a) & 1]
  ad, vaf = _call_values(variant, 'AD'), _call_values(variant, 'VAF')
  if ad is not None and len(ad) == len(variant.alternate_bases) + 1:
    ad = [ad[0]] + [ad[a + 1] for a in keep]
  if vaf is not None and len(vaf) == len(variant.alternate_bases):
    vaf = [vaf[a] for a in keep]
  return [variant.alternate_bases[a] for a in keep], ad, vaf


def simplify_variant_alleles(ref: str, alts: Sequence[str]) -> Tuple[str, List[str]]:
  """Strips the longest common suffix of the reference and every alt, leaving at least one base each."""
  alleles = [ref] + list(alts)
  shortest = min(len(a) for a in alleles)
  strip = 0
  while strip < shortest - 1 and len({a[len(a) - 1 - strip] for a in alleles}) == 1:
    strip += 1
  if not strip:
    return ref, list(alts)
  return ref[:-strip], [a[:-strip] for a in alts]


@dataclasses.dataclass
class VcfRecord:
  reference_name: str
  start: int
  end: int
  reference_bases: str
  alternate_bases: List[str]
  quality: float
  filter: str
  genotype: List[int]
  gq: int
  genotype_likelihood: List[float]
  dp: Optional[int] = None
  ad: Optional[List[int]] = None
  vaf: Optional[List[float]] = None
  call_set_name: str = ''


def add_call_to_variant(variant: T.Variant, predictions: Sequence[float], best: int, removed: int = 0,
                        qual_filter: float = DEFAULT_QUAL_FILTER,
                        cnn_homref_call_min_gq: float = DEFAULT_CNN_HOMREF_CALL_MIN_GQ,
                        sample_name: Optional[str] = None) -> VcfRecord:
  """Step 4 for one site: the merged predictions of its kept alleles -> the finished record."""
  gq, qual = compute_quals(predictions, best)
  genotype = genotype_of_index(best)
  if genotype == [0, 0]:
    filter_name = 'RefCall'
    if gq < cnn_homref_call_min_gq:
      genotype = [-1, -1]
  else:
    filter_name = 'LowQual' if qual < qual_filter else 'PASS'
  gls = [math.log10(max(p, 1.0 - _MAX_CONFIDENCE)) for p in predictions]
  alts, ad, vaf = prune_alleles(variant, removed)
  ref, alts = simplify_variant_alleles(variant.reference_bases, alts)
  dp = _call_values(variant, 'DP')
  name = sample_name if sample_name is not None else (variant.calls[0].call_set_name if variant.calls else '')
  return VcfRecord(reference_name=variant.reference_name, start=variant.start, end=variant.start + len(ref),
                   reference_bases=ref, alternate_bases=alts, quality=qual, filter=filter_name, genotype=genotype,
                   gq=gq, genotype_likelihood=gls, dp=dp[0] if dp else None, ad=ad, vaf=vaf, call_set_name=name)


def finish_sites(variants: Sequence[T.Variant], result: SiteGenotypes, qual_filter: float = DEFAULT_QUAL_FILTER,
                 cnn_homref_call_min_gq: float = DEFAULT_CNN_HOMREF_CALL_MIN_GQ,
                 sample_name: Optional[str] = None) -> List[VcfRecord]:
  """Step 4 for the sites of one native call, whichever side made it."""
  return [add_call_to_variant(v, result.site_predictions(s), int(result.best[s]), int(result.removed[s]), qual_filter,
                              cnn_homref_call_min_gq, sample_name) for s, v in enumerate(variants)]


def merge_predictions(call_variants_outputs, qual_filter: float = DEFAULT_QUAL_FILTER):
  """One site's (variant, alt indices, probabilities) triples, in any order -> (removed alts' bit mask, the merged
  predictions of the kept alleles, the index of the best) by the host code."""
  items = sorted(call_variants_outputs, key=lambda c: (len(c[1]), list(c[1])))
  variant = items[0][0]
  tables = site_tables([(len(variant.alternate_bases), [c[1] for c in items])])
  probs = np.array([c[2] for c in items], np.float32).reshape(-1, 3)
  result = genotype_sites(probs, *tables, qual_filter=qual_filter, already_rounded=True)
  check_status(result, lambda i: probs[i], tables[1], lambda s: describe_variant(variant))
  return int(result.removed[0]), result.site_predictions(0), int(result.best[0])


def describe_variant(variant: T.Variant) -> str:
  return '%s:%d %s>%s' % (variant.reference_name, variant.start + 1, variant.reference_bases,
                          ','.join(variant.alternate_bases))


# ------------------------------------------------------------------------------------------ the VCF writer
_HEADER = (
    '##fileformat=VCFv4.2',
    '##FILTER=<ID=PASS,Description="All filters passed">',
    '##FILTER=<ID=RefCall,Description="Genotyping model thinks this site is reference.">',
    '##FILTER=<ID=LowQual,Description="Confidence in this variant being real is below calling threshold.">',
    '##FORMAT=<ID=GT,Number=1,Type=String,Description="Genotype">',
    '##FORMAT=<ID=GQ,Number=1,Type=Integer,Description="Conditional genotype quality">',
    '##FORMAT=<ID=DP,Number=1,Type=Integer,Description="Read depth">',
    '##FORMAT=<ID=AD,Number=R,Type=Integer,Description="Read depth for each allele">',
    '##FORMAT=<ID=VAF,Number=A,Type=Float,Description="Variant allele fractions.">',
    '##FORMAT=<ID=PL,Number=G,Type=Integer,Description="Phred-scaled genotype likelihoods rounded to the closest integer">',
)


def vcf_header(contigs: Iterable[Tuple[str, int]], sample_name: str, extra: Sequence[str] = ()) -> str:
  lines = list(_HEADER) + list(extra)
  lines += ['##contig=<ID=%s,length=%d>' % (name, length) for name, length in contigs]
  lines.append('\t'.join(['#CHROM', 'POS', 'ID', 'REF', 'ALT', 'QUAL', 'FILTER', 'INFO', 'FORMAT', sample_name]))
  return '\n'.join(lines) + '\n'


def vcf_row(r: VcfRecord) -> str:
  pls = [int(round(-10 * gl)) for gl in r.genotype_likelihood]
  low = min(pls)
  sample = [
      '/'.join('.' if g < 0 else str(g) for g in r.genotype),
      str(r.gq),
      '.' if r.dp is None else str(r.dp),
      '.' if r.ad is None else ','.join(str(v) for v in r.ad),
      '.' if not r.vaf else ','.join('%g' % v for v in r.vaf),
      ','.join(str(pl - low) for pl in pls),
  ]
  return '\t'.join([r.reference_name, str(r.start + 1), '.', r.reference_bases,
                    ','.join(r.alternate_bases) if r.alternate_bases else '.',
                    '%g' % (round(r.quality, 1) + 0.0),     # + 0.0: a phred of -0.0 prints as 0
                    r.filter, '.', 'GT:GQ:DP:AD:VAF:PL', ':'.join(sample)]) + '\n'


def vcf_text(records: Sequence[VcfRecord], contigs: Sequence[Tuple[str, int]], sample_name: str) -> str:
  """Header and rows, the rows sorted by (contig order, start, end), stable."""
  order = {name: k for k, (name, _) in enumerate(contigs)}
  for r in records:
    if r.reference_name not in order:
      raise ValueError('%s is not a contig of the reference' % r.reference_name)
  rows = sorted(records, key=lambda r: (order[r.reference_name], r.start, r.end))
  return vcf_header(contigs, sample_name) + ''.join(vcf_row(r) for r in rows)


def write_vcf(path: str, records: Sequence[VcfRecord], contigs: Sequence[Tuple[str, int]], sample_name: str) -> None:
  _write_text(path, vcf_text(records, contigs, sample_name))


def _write_text(path: str, text: str) -> None:
  """GZIP when the name ends in .gz."""
  _write_bytes(path, text.encode())


def _write_bytes(path: str, *chunks: bytes) -> None:
  """DV_BGZF=1: a .gz name gets BGZF members from the host code (bgzf_compress) instead of one gzip stream."""
  if path.endswith('.gz') and bgzf_switch():
    _write_finished(path, bgzf_compress(b''.join(chunks)))
    return
  with open(path, 'wb') as f:
    if path.endswith('.gz'):
      with gzip.GzipFile(filename='', fileobj=f, mode='wb', mtime=0) as z:     # the same bytes on every run
        for data in chunks:
          z.write(data)
    else:
      for data in chunks:
        f.write(data)


def _write_finished(path: str, data: bytes) -> None:
  """The bytes as they are, whatever the name ends in."""
  with open(path, 'wb') as f:
    f.write(data)


# ------------------------------------------------------------------------------------------ BGZF (section 24)
@dataclasses.dataclass
class BgzfFile:
  """One native call's result (dv_bgzf_view, copied)."""
  data: bytes                       # the members and the end-of-file member
  block_coff: np.ndarray            # int64 [n_blocks + 1]: every member's offset, the end-of-file member's last
  stored_blocks: int


def bgzf_switch() -> bool:
  """DV_BGZF=1: names that end in .gz are written as BGZF."""
  return _env_on('DV_BGZF')


def bgzf_params() -> Dict[str, int]:
  """The constants of csrc/bgzf_deflate.h: block, tile, seg, hash_bits."""
  params = _lib.DvBgzfParameters()
  _lib.check(_lib.lib().dv_bgzf_params(C.byref(params)))
  return {name: int(getattr(params, name)) for name, _ in params._fields_}


def _take_bgzf(handle) -> BgzfFile:
  l = _lib.lib()
  try:
    view = _lib.DvBgzfView()
    _lib.check(l.dv_bgzf_arrays(handle, C.byref(view)))
    coff = np.ctypeslib.as_array(C.cast(view.block_coff, C.POINTER(C.c_int64)), (view.n_blocks + 1,)).copy()
    return BgzfFile(data=C.string_at(view.data, view.n_bytes), block_coff=coff, stored_blocks=int(view.stored_blocks))
  finally:
    l.dv_bgzf_free(handle)


def bgzf_file(data, device: bool = False, stream=None) -> BgzfFile:
  """dv_bgzf_compress, or dv_bgzf_compress_device with `device` (csrc/bgzf.hip).  data: bytes, or with `device` a
  contiguous uint8 torch tensor in device memory, which is read where it lies."""
  l = _lib.lib()
  handle = C.c_void_p()
  if hasattr(data, 'data_ptr'):
    if not device:
      raise ValueError('a tensor is compressed on the device')
    if not data.is_cuda or not data.is_contiguous() or data.element_size() != 1:
      raise ValueError('a contiguous one-byte tensor in device memory is expected')
    if stream is None:        # the library's own stream does not wait for the tensor's
      import torch  # device memory + stream only
      torch.cuda.current_stream(data.device).synchronize()
    _lib.check(l.dv_bgzf_compress_device(C.c_void_p(data.data_ptr() or None), _lib.DV_MEM_DEVICE, data.numel(),
                                         C.byref(handle), C.c_void_p(stream or None)))
    return _take_bgzf(handle)
  data = bytes(data)
  text = C.cast(C.c_char_p(data), C.c_void_p)
  if device:
    _lib.check(l.dv_bgzf_compress_device(text, _lib.DV_MEM_HOST, len(data), C.byref(handle), C.c_void_p(stream or None)))
  else:
    _lib.check(l.dv_bgzf_compress(text, len(data), C.byref(handle)))
  return _take_bgzf(handle)


def bgzf_compress(data, device: bool = False, stream=None) -> bytes:
  """data as a BGZF file: members of at most bgzf_params()['block'] input bytes and the end-of-file member."""
  return bgzf_file(data, device, stream).data


def last_bgzf_stats() -> Dict[str, int]:
  """What the calling thread's last device compression did."""
  stats = _lib.DvBgzfStats()
  _lib.check(_lib.lib().dv_bgzf_last_stats(C.byref(stats)))
  return {name: int(getattr(stats, name)) for name, _ in stats._fields_}


def fasta_contigs(ref_reader) -> List[Tuple[str, int]]:
  return [(name, ref_reader.n_bases(name)) for name in ref_reader.contig_names()]


def default_sample_name(records: Sequence[VcfRecord], sample_name: Optional[str]) -> str:
  if sample_name:
    return sample_name
  for r in records:
    if r.call_set_name:
      return r.call_set_name
  return 'default'


# ------------------------------------------------------------------------------------------ the gVCF merge, native
@dataclasses.dataclass
class MergedBlocks:
  """One call's arrays (dv_gvcf_merged_view, copied): the pieces the variants leave of the blocks, and where every
  piece and every variant stands in the merged sequence of P + V slots."""
  piece_start: np.ndarray    # int64 [P]
  piece_end: np.ndarray      # int64 [P]
  piece_block: np.ndarray    # int32 [P], the index of the source block in the call
  piece_slot: np.ndarray     # int64 [P]
  var_slot: np.ndarray       # int64 [V]


def _merge_arguments(block_off, var_off, block_start, block_end, var_start, var_end):
  arrays = [np.ascontiguousarray(a, np.int64).reshape(-1)
            for a in (block_off, var_off, block_start, block_end, var_start, var_end)]
  b_off, v_off, b_start, b_end, v_start, v_end = arrays
  if b_off.size < 1 or b_off.size != v_off.size:
    raise ValueError('block_off and var_off must have one entry per group and one more')
  if b_start.size != b_end.size or v_start.size != v_end.size:
    raise ValueError('one end per start is expected')
  if int(b_off[-1]) != b_start.size or int(v_off[-1]) != v_start.size:
    raise ValueError('the offsets must end at the number of blocks and of variants')
  return arrays


def _take_merged(handle) -> MergedBlocks:
  l = _lib.lib()
  try:
    view = _lib.DvGvcfMergedView()
    _lib.check(l.dv_gvcf_merged_arrays(handle, C.byref(view)))

    def array(ptr, count, dtype):
      if count == 0:
        return np.zeros(0, dtype)
      return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint8)),
                                   (count * np.dtype(dtype).itemsize,)).view(dtype).copy()
    p, v = view.n_pieces, view.n_variants
    return MergedBlocks(piece_start=array(view.piece_start, p, np.int64), piece_end=array(view.piece_end, p, np.int64),
                        piece_block=array(view.piece_block, p, np.int32),
                        piece_slot=array(view.piece_slot, p, np.int64), var_slot=array(view.var_slot, v, np.int64))
  finally:
    l.dv_gvcf_merged_free(handle)


def merge_blocks_and_variants(block_off, var_off, block_start, block_end, var_start, var_end) -> MergedBlocks:
  """The host code (dv_gvcf_merge).  G groups (contigs): block_off, var_off int64 [G + 1]; per group the blocks
  [start, end) sorted and disjoint, the variants sorted by (start, end)."""
  a = _merge_arguments(block_off, var_off, block_start, block_end, var_start, var_end)
  handle = C.c_void_p()
  _lib.check(_lib.lib().dv_gvcf_merge(a[0].size - 1, *[x.ctypes.data for x in a], C.byref(handle)))
  return _take_merged(handle)


def merge_blocks_and_variants_device(block_off, var_off, block_start, block_end, var_start, var_end,
                                     stream=None) -> MergedBlocks:
  """The same on the device (dv_gvcf_merge_device): one upload, nine launches, one download.  `stream` is a raw
  handle; None = a stream the library owns."""
  a = _merge_arguments(block_off, var_off, block_start, block_end, var_start, var_end)
  handle = C.c_void_p()
  _lib.check(_lib.lib().dv_gvcf_merge_device(a[0].size - 1, *[x.ctypes.data for x in a], C.byref(handle),
                                             C.c_void_p(stream or None)))
  return _take_merged(handle)


def last_merge_stats() -> Dict[str, int]:
  stats = _lib.DvGvcfMergeStats()
  _lib.check(_lib.lib().dv_gvcf_merge_last_stats(C.byref(stats)))
  return {name: int(getattr(stats, name)) for name, _ in stats._fields_}


def merge_scan_chunk() -> int:
  return int(_lib.lib().dv_gvcf_merge_scan_chunk())


# ------------------------------------------------------------------------------------------ the gVCF writer
GVCF_ALT = '<*>'
_GVCF_GL = -99.0          # every genotype that names <*>: PL 990 before the minimum is taken off
_GVCF_HEADER = (
    '##INFO=<ID=END,Number=1,Type=Integer,Description="End position (for use with symbolic alleles)">',
    '##FORMAT=<ID=MIN_DP,Number=1,Type=Integer,Description="Minimum DP observed within the GVCF block.">',
)
_GVCF_HEADER_MED_DP = '##FORMAT=<ID=MED_DP,Number=1,Type=Integer,Description="Median DP observed within the GVCF block rounded to the nearest integer.">'


def gvcf_variant_row(r: VcfRecord) -> str:
  """vcf_row of the record with <*> as one more alt: AD and VAF 0, and GL -99 for its A + 2 genotypes, which follow
  the record's own in VCF order."""
  alts = len(r.alternate_bases)
  if len(r.genotype_likelihood) != (alts + 1) * (alts + 2) // 2:
    raise ValueError('%s:%d: one likelihood per genotype of its alleles is expected' % (r.reference_name, r.start + 1))
  return vcf_row(dataclasses.replace(
      r, alternate_bases=list(r.alternate_bases) + [GVCF_ALT], ad=None if r.ad is None else list(r.ad) + [0],
      vaf=None if r.vaf is None else list(r.vaf) + [0.0],
      genotype_likelihood=list(r.genotype_likelihood) + [_GVCF_GL] * (alts + 2)))


def _gvcf_dtype():
  from deepvariant_amd import allelecounter
  return allelecounter.GVCF_BLOCK_DTYPE


def blocks_from_variants(variants: Iterable[T.Variant]) -> Dict[str, np.ndarray]:
  """Reference-block Variant records (make_gvcfs / variant_calling.gvcf_record, in any order) -> {contig: their
  GVCF_BLOCK_DTYPE array sorted by start}; MED_DP -1 where a record has none."""
  columns: Dict[str, list] = {}
  for v in variants:
    call = v.calls[0]
    gl = list(call.genotype_likelihood)
    if len(gl) != 3 or not v.reference_bases:
      raise ValueError('%s:%d: a reference block carries one base and three likelihoods' % (v.reference_name, v.start + 1))
    med = call.info['MED_DP'].values[0].int_value if 'MED_DP' in call.info else -1
    columns.setdefault(v.reference_name, []).append(
        (v.start, v.end, gl, call.info['GQ'].values[0].int_value, call.info['MIN_DP'].values[0].int_value, med,
         ord(v.reference_bases[0]), 1 if list(call.genotype) == [0, 0] else 0, (0, 0)))
  out = {}
  for contig, rows in columns.items():
    arr = np.array(rows, _gvcf_dtype())
    out[contig] = arr[np.argsort(arr['start'], kind='stable')]
  return out


def _piece_rows(contig: str, blocks: np.ndarray, piece_start: np.ndarray, piece_end: np.ndarray, piece_block: np.ndarray,
                ref_reader, med_dp: bool) -> List[str]:
  """The rows of one contig's pieces, formatted from columns: piece_block indexes `blocks`."""
  if not piece_start.size:
    return []
  src = blocks[piece_block]
  bases = src['ref_base'].copy()
  moved = np.nonzero(piece_start != src['start'])[0]
  if moved.size:
    # one fetch per contig over the moved starts, indexed by array
    lo, hi = int(piece_start[moved].min()), int(piece_start[moved].max()) + 1
    fetched = np.frombuffer(ref_reader.get_bases(contig, lo, hi).encode(), np.uint8)
    bases[moved] = fetched[piece_start[moved] - lo]
  pls = np.rint(-10.0 * src['likelihoods']).astype(np.int64)       # vcf_row's int(round(-10 * GL)): half to even
  pls -= pls.min(axis=1, keepdims=True)
  letters = bases.tobytes().decode('latin-1')
  head = contig + '\t'
  rows = []
  if med_dp:
    tail = '\tGT:GQ:MIN_DP:MED_DP:PL\t'
    for k, (s, e, gq, mn, md, ok, (p0, p1, p2)) in enumerate(zip(
        (piece_start + 1).tolist(), piece_end.tolist(), src['gq'].tolist(), src['min_dp'].tolist(),
        src['med_dp'].tolist(), src['has_valid_gl'].tolist(), pls.tolist())):
      rows.append('%s%d\t.\t%s\t<*>\t0\t.\tEND=%d%s%s:%d:%d:%s:%d,%d,%d\n' % (
          head, s, letters[k], e, tail, '0/0' if ok else './.', gq, mn, '.' if md < 0 else md, p0, p1, p2))
  else:
    tail = '\tGT:GQ:MIN_DP:PL\t'
    for k, (s, e, gq, mn, ok, (p0, p1, p2)) in enumerate(zip(
        (piece_start + 1).tolist(), piece_end.tolist(), src['gq'].tolist(), src['min_dp'].tolist(),
        src['has_valid_gl'].tolist(), pls.tolist())):
      rows.append('%s%d\t.\t%s\t<*>\t0\t.\tEND=%d%s%s:%d:%d:%d,%d,%d\n' % (
          head, s, letters[k], e, tail, '0/0' if ok else './.', gq, mn, p0, p1, p2))
  return rows


def gvcf_rows(records: Sequence[VcfRecord], blocks_by_contig: Dict[str, np.ndarray], ref_reader,
              contigs: Sequence[Tuple[str, int]], device: bool = False, stream=None) -> Tuple[List[str], bool]:
  """-> (the rows of the gVCF in merged order, the contigs in the order of `contigs`; whether the blocks carry
  MED_DP).  records: the finished records, in any order.  blocks_by_contig: GVCF_BLOCK_DTYPE arrays, in any order.
  One native merge call over all contigs: the host code, or the device with `device`."""
  order = {name: k for k, (name, _) in enumerate(contigs)}
  for name in list(blocks_by_contig) + [r.reference_name for r in records]:
    if name not in order:
      raise ValueError('%s is not a contig of the reference' % name)
  records = sorted(records, key=lambda r: (order[r.reference_name], r.start, r.end))
  dtype = _gvcf_dtype()
  blocks, block_off, var_off = [], [0], [0]
  at = 0
  for name, _ in contigs:
    arr = np.asarray(blocks_by_contig.get(name, np.zeros(0, dtype)), dtype)
    if arr.size > 1 and (arr['start'][1:] < arr['start'][:-1]).any():
      arr = arr[np.argsort(arr['start'], kind='stable')]
    blocks.append(arr)
    block_off.append(block_off[-1] + arr.size)
    while at < len(records) and records[at].reference_name == name:
      at += 1
    var_off.append(at)
  every = np.concatenate(blocks) if blocks else np.zeros(0, dtype)
  var_start = np.array([r.start for r in records], np.int64)
  var_end = np.array([r.end for r in records], np.int64)
  merge = merge_blocks_and_variants_device if device else merge_blocks_and_variants
  kwargs = {'stream': stream} if device else {}
  merged = merge(block_off, var_off, every['start'], every['end'], var_start, var_end, **kwargs)
  med_dp = bool(every.size and (every['med_dp'] >= 0).any())
  rows: List[Optional[str]] = [None] * (merged.piece_slot.size + len(records))
  piece_group = np.searchsorted(merged.piece_block, np.array(block_off, np.int64), side='left')
  for g, (name, _) in enumerate(contigs):
    p0, p1 = int(piece_group[g]), int(piece_group[g + 1])
    texts = _piece_rows(name, blocks[g], merged.piece_start[p0:p1], merged.piece_end[p0:p1],
                        merged.piece_block[p0:p1].astype(np.int64) - block_off[g], ref_reader, med_dp)
    for slot, text in zip(merged.piece_slot[p0:p1].tolist(), texts):
      rows[slot] = text
  for slot, r in zip(merged.var_slot.tolist(), records):
    rows[slot] = gvcf_variant_row(r)
  if any(row is None for row in rows):
    raise RuntimeError('the merged slots are not a permutation')
  return rows, med_dp


def gvcf_text(records: Sequence[VcfRecord], blocks_by_contig: Dict[str, np.ndarray], ref_reader,
              contigs: Sequence[Tuple[str, int]], sample_name: str, device: bool = False, stream=None,
              rows: str = 'python') -> str:
  """rows: 'python' formats the rows here (gvcf_rows); 'native' takes them from gvcf_body_native (section 23)."""
  if rows == 'native':
    header, body = _native_gvcf(records, blocks_by_contig, ref_reader, contigs, sample_name, device, stream)
    return header + body.decode()
  if rows != 'python':
    raise ValueError("rows must be 'python' or 'native'")
  rows, med_dp = gvcf_rows(records, blocks_by_contig, ref_reader, contigs, device, stream)
  extra = _GVCF_HEADER + ((_GVCF_HEADER_MED_DP,) if med_dp else ())
  return vcf_header(contigs, sample_name, extra) + ''.join(rows)


def write_gvcf(path: str, records: Sequence[VcfRecord], blocks_by_contig: Dict[str, np.ndarray], ref_reader,
               contigs: Sequence[Tuple[str, int]], sample_name: str, device: bool = False, stream=None,
               rows: str = 'python') -> None:
  """The .gz rule is write_vcf's.  rows as for gvcf_text; the native body goes to the file as the bytes it is."""
  if rows == 'native' and path.endswith('.gz') and bgzf_switch():
    _write_finished(path, gvcf_file_native(records, blocks_by_contig, ref_reader, contigs, sample_name, device,
                                           stream).file.data)
    return
  if rows == 'native':
    header, body = _native_gvcf(records, blocks_by_contig, ref_reader, contigs, sample_name, device, stream)
    _write_bytes(path, header.encode(), body)
    return
  _write_text(path, gvcf_text(records, blocks_by_contig, ref_reader, contigs, sample_name, device, stream, rows))


# ------------------------------------------------------------------------------------------ the gVCF rows, native
@dataclasses.dataclass
class GvcfBody:
  """One native call's result (dv_gvcf_text_view, copied): the rows of a gVCF in merged order, without the header."""
  text: bytes
  row_off: Optional[np.ndarray]     # int64 [rows + 1] when asked for
  med_dp: bool                      # the block rows carry MED_DP
  n_pieces: int                     # the block rows; the others are the variants'


def gvcf_rows_native(block_off, var_off, blocks, var_start, var_end, var_end_base, var_text_off, var_text: bytes,
                     name_off, names: bytes, med_dp: int = -1, want_row_off: bool = False, device: bool = False,
                     stream=None) -> GvcfBody:
  """dv_gvcf_rows, or dv_gvcf_rows_device with `device` (csrc/gvcf_rows.hip): the merge of merge_blocks_and_variants
  carried on to the text.  blocks: GVCF_BLOCK_DTYPE [B] over all groups; var_end_base: uint8 [V], the reference base at
  every variant's end; var_text_off [V + 1] into var_text, the variants' finished rows; name_off [G + 1] into names,
  the groups' contig names; med_dp: -1 = MED_DP when any block has one, else 0 or 1."""
  arg, _alive = _rows_input(block_off, var_off, blocks, var_start, var_end, var_end_base, var_text_off, var_text, name_off,
                            names, med_dp, want_row_off)
  l = _lib.lib()
  handle = C.c_void_p()
  if device:
    _lib.check(l.dv_gvcf_rows_device(C.byref(arg), C.byref(handle), C.c_void_p(stream or None)))
  else:
    _lib.check(l.dv_gvcf_rows(C.byref(arg), C.byref(handle)))
  try:
    view = _lib.DvGvcfTextView()
    _lib.check(l.dv_gvcf_text_arrays(handle, C.byref(view)))
    row_off = None
    if want_row_off:
      row_off = np.ctypeslib.as_array(C.cast(view.row_off, C.POINTER(C.c_int64)), (view.n_rows + 1,)).copy()
    return GvcfBody(text=C.string_at(view.text, view.n_bytes), row_off=row_off, med_dp=bool(view.med_dp),
                    n_pieces=int(view.n_pieces))
  finally:
    l.dv_gvcf_text_free(handle)


def _rows_input(block_off, var_off, blocks, var_start, var_end, var_end_base, var_text_off, var_text: bytes, name_off,
                names: bytes, med_dp: int, want_row_off: bool):
  """-> (a dv_gvcf_rows_input, what its pointers point into)."""
  ints = [np.ascontiguousarray(a, np.int64).reshape(-1) for a in (block_off, var_off, var_start, var_end, var_text_off,
                                                                  name_off)]
  b_off, v_off, v_start, v_end, text_off, n_off = ints
  blocks = np.ascontiguousarray(blocks, _gvcf_dtype()).reshape(-1)
  bases = np.ascontiguousarray(var_end_base, np.uint8).reshape(-1)
  if b_off.size < 1 or b_off.size != v_off.size or n_off.size != b_off.size:
    raise ValueError('block_off, var_off and name_off must have one entry per group and one more')
  if v_start.size != v_end.size or bases.size != v_start.size or text_off.size != v_start.size + 1:
    raise ValueError('one end, one base and one row per variant are expected')
  if int(b_off[-1]) != blocks.size or int(v_off[-1]) != v_start.size:
    raise ValueError('the offsets must end at the number of blocks and of variants')
  if int(text_off[-1]) > len(var_text) or int(n_off[-1]) > len(names):
    raise ValueError('the text offsets pass the end of their text')
  arg = _lib.DvGvcfRowsInput(
      n_groups=b_off.size - 1, med_dp=int(med_dp), want_row_off=1 if want_row_off else 0, block_off=b_off.ctypes.data,
      var_off=v_off.ctypes.data, blocks=blocks.ctypes.data, var_start=v_start.ctypes.data, var_end=v_end.ctypes.data,
      var_end_base=bases.ctypes.data, var_text_off=text_off.ctypes.data,
      var_text=C.cast(C.c_char_p(var_text), C.c_void_p), name_off=n_off.ctypes.data,
      names=C.cast(C.c_char_p(names), C.c_void_p))
  return arg, (ints, blocks, bases, var_text, names)


@dataclasses.dataclass
class GvcfFile:
  """One dv_gvcf_rows_bgzf[_device] call's result: the compressed gVCF and what its text was."""
  file: BgzfFile
  text_bytes: int                   # the prefix and the rows
  n_rows: int
  n_pieces: int
  row_off: Optional[np.ndarray]     # int64 [rows + 1] into prefix + rows when asked for


def gvcf_rows_bgzf_native(prefix: bytes, block_off, var_off, blocks, var_start, var_end, var_end_base, var_text_off,
                          var_text: bytes, name_off, names: bytes, med_dp: int, want_row_off: bool = False,
                          device: bool = False, stream=None) -> GvcfFile:
  """gvcf_rows_native's rows behind `prefix`, compressed by the same call (section 24): on the device the text is
  deflated where the rows were written and only the file comes back.  med_dp: 0 or 1, as the prefix says."""
  arg, _alive = _rows_input(block_off, var_off, blocks, var_start, var_end, var_end_base, var_text_off, var_text, name_off,
                            names, med_dp, want_row_off)
  l = _lib.lib()
  handle, meta = C.c_void_p(), _lib.DvGvcfRowsMeta()
  lead = C.cast(C.c_char_p(prefix), C.c_void_p)
  if device:
    _lib.check(l.dv_gvcf_rows_bgzf_device(C.byref(arg), lead, len(prefix), C.byref(meta), C.byref(handle),
                                          C.c_void_p(stream or None)))
  else:
    _lib.check(l.dv_gvcf_rows_bgzf(C.byref(arg), lead, len(prefix), C.byref(meta), C.byref(handle)))
  row_off = None
  if want_row_off:          # the handle owns it: copy before _take_bgzf frees the handle
    row_off = np.ctypeslib.as_array(C.cast(meta.row_off, C.POINTER(C.c_int64)), (meta.n_rows + 1,)).copy()
  return GvcfFile(file=_take_bgzf(handle), text_bytes=int(meta.text_bytes), n_rows=int(meta.n_rows),
                  n_pieces=int(meta.n_pieces), row_off=row_off)


def last_rows_stats() -> Dict[str, int]:
  """What the calling thread's last device call of gvcf_rows_native did."""
  stats = _lib.DvGvcfRowsStats()
  _lib.check(_lib.lib().dv_gvcf_rows_last_stats(C.byref(stats)))
  return {name: int(getattr(stats, name)) for name, _ in stats._fields_}


def gvcf_body_native(records: Sequence[VcfRecord], blocks_by_contig: Dict[str, np.ndarray], ref_reader,
                     contigs: Sequence[Tuple[str, int]], device: bool = False, stream=None,
                     want_row_off: bool = False) -> GvcfBody:
  """gvcf_rows with the block rows made by the native code, on the host or with `device` on the device: the records
  and blocks are sorted and grouped as there, the variants' rows are gvcf_variant_row's, and one native call merges
  and prints.  One get_bases per contig that has variants, over the variant ends below the contig's length."""
  return gvcf_rows_native(**_native_arguments(records, blocks_by_contig, ref_reader, contigs), want_row_off=want_row_off,
                          device=device, stream=stream)


def _native_arguments(records, blocks_by_contig, ref_reader, contigs) -> dict:
  """gvcf_rows_native's arrays for the records and blocks of a gVCF."""
  order = {name: k for k, (name, _) in enumerate(contigs)}
  for name in list(blocks_by_contig) + [r.reference_name for r in records]:
    if name not in order:
      raise ValueError('%s is not a contig of the reference' % name)
  records = sorted(records, key=lambda r: (order[r.reference_name], r.start, r.end))
  dtype = _gvcf_dtype()
  blocks, block_off, var_off, name_off, names = [], [0], [0], [0], []
  var_end = np.array([r.end for r in records], np.int64)
  var_end_base = np.full(len(records), ord('N'), np.uint8)      # an end at the contig's length: no piece starts there
  at = 0
  for name, length in contigs:
    arr = np.asarray(blocks_by_contig.get(name, np.zeros(0, dtype)), dtype)
    if arr.size > 1 and (arr['start'][1:] < arr['start'][:-1]).any():
      arr = arr[np.argsort(arr['start'], kind='stable')]
    blocks.append(arr)
    block_off.append(block_off[-1] + arr.size)
    first = at
    while at < len(records) and records[at].reference_name == name:
      at += 1
    var_off.append(at)
    names.append(name.encode())
    name_off.append(name_off[-1] + len(names[-1]))
    inside = first + np.nonzero(var_end[first:at] < length)[0]
    if inside.size:
      lo, hi = int(var_end[inside].min()), int(var_end[inside].max()) + 1
      fetched = np.frombuffer(ref_reader.get_bases(name, lo, hi).encode('latin-1'), np.uint8)
      var_end_base[inside] = fetched[var_end[inside] - lo]
  texts = [gvcf_variant_row(r).encode() for r in records]
  var_text_off = np.zeros(len(texts) + 1, np.int64)
  np.cumsum([len(t) for t in texts], out=var_text_off[1:])
  return dict(block_off=block_off, var_off=var_off, blocks=np.concatenate(blocks) if blocks else np.zeros(0, dtype),
              var_start=np.array([r.start for r in records], np.int64), var_end=var_end, var_end_base=var_end_base,
              var_text_off=var_text_off, var_text=b''.join(texts), name_off=name_off, names=b''.join(names))


def gvcf_file_native(records: Sequence[VcfRecord], blocks_by_contig: Dict[str, np.ndarray], ref_reader,
                     contigs: Sequence[Tuple[str, int]], sample_name: str, device: bool = False, stream=None,
                     want_row_off: bool = False) -> GvcfFile:
  """The whole .g.vcf.gz from one native call: the header goes in as the prefix, so whether it names MED_DP is
  decided here, as gvcf_rows decides it."""
  args = _native_arguments(records, blocks_by_contig, ref_reader, contigs)
  med_dp = bool((args['blocks']['med_dp'] >= 0).any())
  header = vcf_header(contigs, sample_name, _GVCF_HEADER + ((_GVCF_HEADER_MED_DP,) if med_dp else ()))
  return gvcf_rows_bgzf_native(header.encode(), med_dp=int(med_dp), want_row_off=want_row_off, device=device,
                               stream=stream, **args)


def _native_gvcf(records, blocks_by_contig, ref_reader, contigs, sample_name, device, stream) -> Tuple[str, bytes]:
  body = gvcf_body_native(records, blocks_by_contig, ref_reader, contigs, device, stream)
  extra = _GVCF_HEADER + ((_GVCF_HEADER_MED_DP,) if body.med_dp else ())
  return vcf_header(contigs, sample_name, extra), body.text


def concatenate_blocks(arrays_by_contig: Dict[str, List[np.ndarray]]) -> Dict[str, np.ndarray]:
  """{contig: [the regions' block arrays]} -> {contig: one array}."""
  return {name: np.concatenate(arrays) for name, arrays in arrays_by_contig.items() if arrays}


def _env_on(name: str) -> bool:
  return os.environ.get(name, '0') not in ('', '0')


def gvcf_rows_switch() -> str:
  """DV_GVCF_ROWS_NATIVE=1: both gVCF routes pass rows='native'; the side follows the merge's switches."""
  return 'native' if _env_on('DV_GVCF_ROWS_NATIVE') else 'python'


def fused_merge_on_device() -> bool:
  """make_examples --gvcf_outfile: the merge runs on the device; DV_GVCF_MERGE_HOST=1 forces the host code (A/B)."""
  return not _env_on('DV_GVCF_MERGE_HOST')


# ------------------------------------------------------------------------------------------ CVO records -> VCF
def records_from_cvos(cvos, qual_filter: float = DEFAULT_QUAL_FILTER,
                      cnn_homref_call_min_gq: float = DEFAULT_CNN_HOMREF_CALL_MIN_GQ,
                      sample_name: Optional[str] = None) -> List[VcfRecord]:
  """Decoded CallVariantsOutputs (variant, alt indices, probabilities) in any order -> the finished records of their
  sites.  A site is the records that share (contig, start, end, ref, alts); the host code merges them all at once."""
  groups: Dict[tuple, list] = {}
  for variant, alts, probs in cvos:
    if len(probs) != 3:
      raise ValueError('%s: three genotype probabilities are expected' % describe_variant(variant))
    key = (variant.reference_name, variant.start, variant.end, variant.reference_bases, tuple(variant.alternate_bases))
    groups.setdefault(key, []).append((variant, sorted(set(alts)), probs))
  keys = sorted(groups)
  variants, sites, rows = [], [], []
  for key in keys:
    items = sorted(groups[key], key=lambda c: (len(c[1]), c[1]))
    variants.append(items[0][0])
    sites.append((len(key[4]), [c[1] for c in items]))
    rows.extend(c[2] for c in items)
  if not variants:
    return []
  tables = site_tables(sites)
  probs = np.array(rows, np.float32).reshape(-1, 3)
  result = genotype_sites(probs, *tables, qual_filter=qual_filter, already_rounded=True)
  check_status(result, lambda i: probs[i], tables[1], lambda s: describe_variant(variants[s]))
  return finish_sites(variants, result, qual_filter, cnn_homref_call_min_gq, sample_name)


def read_nonvariant_blocks(spec: str) -> Dict[str, np.ndarray]:
  """--nonvariant_site_tfrecord_path: a sharded spec (or one file) of nucleus Variant records, one per reference block
  -> {contig: GVCF_BLOCK_DTYPE array}.  A record is decoded, copied into its row and dropped."""
  from deepvariant_amd import call_variants, protowire, tfrecord
  def decoded():
    for path in call_variants.sharded_paths(spec):
      for rec in tfrecord.read_tfrecords(path):
        yield protowire.decode_variant(rec)
  return blocks_from_variants(decoded())


def postprocess_variants(infile: str, ref: str, outfile: str, qual_filter: float = DEFAULT_QUAL_FILTER,
                         cnn_homref_call_min_gq: float = DEFAULT_CNN_HOMREF_CALL_MIN_GQ,
                         sample_name: Optional[str] = None, nonvariant_site_tfrecord_path: str = '',
                         gvcf_outfile: str = '') -> int:
  """-> the number of rows written to `outfile`.  With the two gVCF arguments (each needs the other) the reference
  blocks are merged with the records and written to `gvcf_outfile`: by the host code, or on the device with
  DV_GVCF_MERGE_DEVICE=1; with DV_GVCF_ROWS_NATIVE=1 the native code of that side prints the rows as well."""
  from deepvariant_amd import call_variants, genomics_io, protowire, tfrecord
  if bool(nonvariant_site_tfrecord_path) != bool(gvcf_outfile):
    raise ValueError('--nonvariant_site_tfrecord_path and --gvcf_outfile need each other')
  cvos = []
  for path in call_variants.sharded_paths(infile):
    for rec in tfrecord.read_tfrecords(path):
      cvos.append(protowire.decode_call_variants_output(rec))
  records = records_from_cvos(cvos, qual_filter, cnn_homref_call_min_gq, sample_name)
  ref_reader = genomics_io.FastaReader(ref)
  contigs, name = fasta_contigs(ref_reader), default_sample_name(records, sample_name)
  write_vcf(outfile, records, contigs, name)
  if gvcf_outfile:
    write_gvcf(gvcf_outfile, records, read_nonvariant_blocks(nonvariant_site_tfrecord_path), ref_reader, contigs, name,
               device=_env_on('DV_GVCF_MERGE_DEVICE'), rows=gvcf_rows_switch())
  return len(records)


def build_arg_parser():
  import argparse
  ap = argparse.ArgumentParser(prog='postprocess_variants', allow_abbrev=False,
                               description='MI355X postprocess_variants: CallVariantsOutput TFRecords -> VCF')
  ap.add_argument('--infile', required=True)
  ap.add_argument('--ref', required=True)
  ap.add_argument('--outfile', required=True)
  ap.add_argument('--qual_filter', type=float, default=DEFAULT_QUAL_FILTER)
  ap.add_argument('--cnn_homref_call_min_gq', type=float, default=DEFAULT_CNN_HOMREF_CALL_MIN_GQ)
  ap.add_argument('--sample_name', default=None)
  # the reference's flag names: the gVCF TFRecords of make_examples --gvcf (GvcfShardWriter here) and the .g.vcf
  ap.add_argument('--nonvariant_site_tfrecord_path', default='')
  ap.add_argument('--gvcf_outfile', default='')
  return ap


def main(argv=None) -> int:
  args = build_arg_parser().parse_args(argv)
  n = postprocess_variants(args.infile, args.ref, args.outfile, args.qual_filter, args.cnn_homref_call_min_gq,
                           args.sample_name, args.nonvariant_site_tfrecord_path, args.gvcf_outfile)
  print('postprocess_variants: wrote %d records' % n)
  return 0


if __name__ == '__main__':
  import sys
  sys.exit(main())
