"""Host mirror of the reference's threshold candidate caller, single-sample form.

  VariantCaller(options)                       deepvariant/variant_calling.h:98-240
  .call_variant(allele_count)                  deepvariant/variant_calling.cc:622-671 (CallVariant)
  .calls_from_allele_counts(allele_counts)     :370-382
  .calls_from_allele_counter(counter)          :365-368
  select_alt_alleles / is_good_alt_allele      :232-258
  calc_ref_bases / make_alt_allele / build_allele_map / add_read_depths / add_supporting_reads
                                               :165-230, :260-340, :673-713

It consumes the AlleleCounts the device counter produces (deepvariant_amd/allelecounter.py) and
emits DeepVariantCall objects with the allele_support read-name lists the pileup encoder's
support channel is computed from -- the candidates of make_examples' "calling" mode for one
sample.  With one sample, no complex-allele creation and no methylation-aware options the
multi-sample caller the reference runs in production (variant_calling_multisample.cc) reduces
to exactly these rules (AlleleFilter :264-311 falls back to IsGoodAltAllele when there is no
other sample).  Not restated: multi-sample filtering, complex alleles, reference-site
sampling (fraction_reference_sites_to_emit), methylation statistics, CallsFromVcf.

gVCF reference confidence (deepvariant/variant_caller.py VariantCaller.reference_confidence /
make_gvcfs with nucleus genomics_math.normalize_log10_probs / log10_ptrue_to_phred):
`site_reference_confidence` is the one restatement of the per-site model; `reference_confidence_table`
tabulates it for the device pass (allelecounter.AlleleCounter.gvcf_blocks) and `make_gvcfs` merges
sites into blocks on the host -- the checker, and the route for callers that hold Python counts.
Which points of it rest on memory rather than the reference's source: DESIGN.md section 9.

Candidates on the device: when the allele counter offers `candidates` /
`candidate_positions` (allelecounter.AlleleCounter over deepvariant_amd/csrc/candidates.hip),
calls_from_allele_counter / call_positions_from_allele_counter take the sites the device selected and
build DeepVariantCalls for those only.  call_variant / calls_from_allele_counts / select_alt_alleles
stay the restatement of the rules, the checker of the device route, and the route for callers that
hold Python counts.
"""
from __future__ import annotations

import functools
import math
import statistics
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from deepvariant_amd import allelecounter as ac
from deepvariant_amd import dv_types as T

K_SUPPORTING_UNCALLED_ALLELE = 'UNCALLED_ALLELE'
K_NO_ALT_ALLELE = '.'
_CANONICAL = frozenset('ACGT')
# reference bases that are IUPAC codes but not A/C/G/T: their sites get no gVCF record
_IUPAC_NON_CANONICAL = frozenset('NRYKMSWBDHV')
GVCF_ALT_ALLELE = '<*>'                   # vcf_constants.GVCF_ALT_ALLELE
GVCF_SITE_DTYPE = np.dtype([('likelihoods', '<f8', (3,)), ('gq', '<i4'), ('has_valid_gl', '<i4')])   # dv_gvcf_site


def site_reference_confidence(n_ref: int, n_total: int, p_error: float,
                              max_gq: int) -> Tuple[int, Tuple[float, float, float]]:
  """VariantCaller._calc_reference_confidence for ploidy 2: -> (raw GQ, normalised log10 likelihoods of
  hom-ref, het, hom-alt).  The whole per-site model is here; everything else (the table, the device
  pass, make_gvcfs) reads it."""
  if n_ref < 0 or n_total < n_ref:
    raise ValueError('Invalid read counts: n_ref=%d n_total=%d' % (n_ref, n_total))
  n_alt = n_total - n_ref
  logp = math.log10(p_error)
  log1p = math.log10(1 - p_error)
  raw = (n_ref * log1p + n_alt * logp, -n_total * math.log10(2), n_ref * logp + n_alt * log1p)
  # genomics_math.normalize_log10_probs: minus log10-sum-exp (max-shifted), clipped at 0
  m = max(raw)
  lse = m + math.log10(sum(math.pow(10.0, x - m) for x in raw))
  lp = tuple(min(x - lse, 0.0) for x in raw)
  # genomics_math.log10_ptrue_to_phred(lp[0], max_gq): the cap when 1 - 10^lp[0] is 0
  ptrue = math.pow(10.0, lp[0])
  phred = max_gq if ptrue == 1 else -10.0 * math.log10(1.0 - ptrue)
  return int(min(math.floor(phred), max_gq)), lp


@functools.lru_cache(maxsize=8)
def reference_confidence_table(p_error: float, max_gq: int, max_cache_coverage: int) -> np.ndarray:
  """The cache of the reference's VariantCaller over 0 <= n_ref <= n_total <= M, as the dv_gvcf_site
  array the device reads: entry n_total * (n_total + 1) // 2 + n_ref.  Computed once per argument set;
  callers must not modify it."""
  m = int(max_cache_coverage)
  table = np.zeros((m + 1) * (m + 2) // 2, GVCF_SITE_DTYPE)
  for t in range(m + 1):
    for r in range(t + 1):
      gq, lp = site_reference_confidence(r, t, p_error, max_gq)
      e = table[t * (t + 1) // 2 + r]
      e['likelihoods'] = lp
      e['gq'] = gq
      e['has_valid_gl'] = int(max(lp) == lp[0])
  return table


def rescale_read_counts_if_necessary(n_ref: int, n_total: int, max_allowed_reads: int) -> Tuple[int, int]:
  """_rescale_read_counts_if_necessary: deeper sites are scaled down to max_allowed_reads."""
  if n_total > max_allowed_reads:
    ratio = n_ref / (1.0 * n_total)
    n_ref = int(math.ceil(ratio * max_allowed_reads))
    n_total = max_allowed_reads
  return n_ref, n_total


def quantize_gq(raw_gq: int, binsize: int) -> int:
  """_quantize_gq: 0, or the lower edge (1, 1 + binsize, ...) of raw_gq's bin."""
  if raw_gq < 1:
    return 0
  return ((raw_gq - 1) // binsize) * binsize + 1


def gvcf_record(reference_name: str, start: int, end: int, ref_base: str, likelihoods, gq: int, min_dp: int,
                med_dp: Optional[int], has_valid_gl: bool, sample_name: str) -> T.Variant:
  """One reference block as make_gvcfs yields it (host and device routes build it here)."""
  call = T.VariantCall(call_set_name=sample_name, genotype=[0, 0] if has_valid_gl else [-1, -1],
                       genotype_likelihood=[float(x) for x in likelihoods])
  call.info['GQ'] = T.ListValue(values=[T.Value(int_value=int(gq))])
  call.info['MIN_DP'] = T.ListValue(values=[T.Value(int_value=int(min_dp))])
  if med_dp is not None:
    call.info['MED_DP'] = T.ListValue(values=[T.Value(int_value=int(med_dp))])
  return T.Variant(reference_name=reference_name, start=int(start), end=int(end), reference_bases=ref_base,
                   alternate_bases=[GVCF_ALT_ALLELE], calls=[call])


def _summary_fields(s):
  """AlleleCountSummary-like object or AlleleCounter.summary_counts tuple -> its five fields."""
  if isinstance(s, tuple):
    return s
  return (s.reference_name, s.position, s.ref_base, s.ref_supporting_read_count, s.total_read_count)


class VariantCallerOptions:
  def __init__(self, min_count_snps=0, min_count_indels=0, min_fraction_snps=0.0, min_fraction_indels=0.0,
               sample_name='', fraction_reference_sites_to_emit=0.0, track_ref_reads=False,
               p_error=0.001, max_gq=50, gq_resolution=5, ploidy=2, max_cache_coverage=100):
    self.min_count_snps, self.min_count_indels = min_count_snps, min_count_indels
    self.min_fraction_snps, self.min_fraction_indels = min_fraction_snps, min_fraction_indels
    self.sample_name = sample_name
    self.fraction_reference_sites_to_emit = fraction_reference_sites_to_emit
    self.track_ref_reads = track_ref_reads
    # gVCF (the values oracle/oracle.py passes to the reference's VariantCallerOptions; M: DESIGN.md section 9)
    self.p_error, self.max_gq, self.gq_resolution, self.ploidy = p_error, max_gq, gq_resolution, ploidy
    self.max_cache_coverage = max_cache_coverage


class GvcfOptions:
  """What the device gVCF pass needs (dv_gvcf_options) plus the call's sample name."""

  def __init__(self, sample_name: str = '', p_error: float = 0.001, max_gq: int = 50, gq_resolution: int = 5,
               max_cache_coverage: int = 100, include_med_dp: bool = False, left_padding: int = 0,
               right_padding: int = 0):
    if gq_resolution < 1:
      raise ValueError('gq_resolution must be >= 1')
    self.sample_name = sample_name
    self.p_error, self.max_gq, self.gq_resolution = float(p_error), int(max_gq), int(gq_resolution)
    self.max_cache_coverage, self.include_med_dp = int(max_cache_coverage), bool(include_med_dp)
    self.left_padding, self.right_padding = int(left_padding), int(right_padding)

  @classmethod
  def from_caller_options(cls, options: VariantCallerOptions, include_med_dp: bool = False, left_padding: int = 0,
                          right_padding: int = 0) -> 'GvcfOptions':
    return cls(options.sample_name, options.p_error, options.max_gq, options.gq_resolution,
               options.max_cache_coverage, include_med_dp, left_padding, right_padding)

  def table(self) -> np.ndarray:
    return reference_confidence_table(self.p_error, self.max_gq, self.max_cache_coverage)

  def key(self) -> tuple:
    return (self.sample_name, self.p_error, self.max_gq, self.gq_resolution, self.max_cache_coverage,
            self.include_med_dp, self.left_padding, self.right_padding)


class CandidateOptions:
  """What the device candidate pass needs (dv_candidate_options): the caller's thresholds, with the
  fractions rounded to float32 as the reference's proto fields are."""

  def __init__(self, min_count_snps: int = 0, min_count_indels: int = 0, min_fraction_snps: float = 0.0,
               min_fraction_indels: float = 0.0, track_ref_reads: bool = False, positions_only: bool = False):
    for value in (min_count_snps, min_count_indels, min_fraction_snps, min_fraction_indels):
      if value < 0:
        raise ValueError('candidate thresholds must be >= 0')
    self.min_count_snps, self.min_count_indels = int(min_count_snps), int(min_count_indels)
    self.min_fraction_snps = float(np.float32(min_fraction_snps))
    self.min_fraction_indels = float(np.float32(min_fraction_indels))
    self.track_ref_reads, self.positions_only = bool(track_ref_reads), bool(positions_only)

  @classmethod
  def from_caller_options(cls, options: VariantCallerOptions, positions_only: bool = False) -> 'CandidateOptions':
    return cls(options.min_count_snps, options.min_count_indels, options.min_fraction_snps,
               options.min_fraction_indels, options.track_ref_reads, positions_only)

  def _with(self, positions_only: bool) -> 'CandidateOptions':
    if self.positions_only == positions_only:
      return self
    return CandidateOptions(self.min_count_snps, self.min_count_indels, self.min_fraction_snps,
                            self.min_fraction_indels, self.track_ref_reads, positions_only)

  def positions_form(self) -> 'CandidateOptions':
    return self._with(True)

  def calls_form(self) -> 'CandidateOptions':
    return self._with(False)

  def key(self) -> tuple:
    """What the selection depends on (a full pass answers a positions query with the same key)."""
    return (self.min_count_snps, self.min_count_indels, self.min_fraction_snps, self.min_fraction_indels)


def _deletion_size(allele) -> int:
  return len(allele.bases) if allele.type == ac.DELETION else -1


def calc_ref_bases(ref_bases: str, alt_alleles: Sequence) -> str:
  """CalcRefBases (:165-191): the longest deletion decides the variant's reference bases."""
  if not alt_alleles:
    return ref_bases
  longest = alt_alleles[0]
  for a in alt_alleles[1:]:               # std::max_element: the FIRST of equal maxima
    if _deletion_size(longest) < _deletion_size(a):
      longest = a
  if longest.type != ac.DELETION:
    return ref_bases
  if len(longest.bases) <= 1:
    raise ValueError('Saw invalid deletion allele with too few bases')
  return ref_bases + longest.bases[1:]


def make_alt_allele(prefix: str, variant_ref: str, from_: int) -> str:
  """MakeAltAllele (:224-229)."""
  return prefix + (variant_ref[from_:] if from_ < len(variant_ref) else '')


def _allele_order(allele):
  return (allele.type, allele.bases)        # OrderAllele, variant_calling.h:83-94


def build_allele_map(alt_alleles: Sequence, ref_bases: str) -> Dict:
  """BuildAlleleMap (:260-296) -> {(type, bases): variant allele}, iterated in OrderAllele order."""
  out = {}
  for a in sorted(alt_alleles, key=_allele_order):
    if a.type in (ac.SUBSTITUTION, ac.INSERTION):
      out[_allele_order(a)] = make_alt_allele(a.bases, ref_bases, 1)
    elif a.type == ac.DELETION:
      if len(a.bases) <= 1:
        raise ValueError('Saw invalid deletion allele with too few bases')
      out[_allele_order(a)] = make_alt_allele(a.bases[:1], ref_bases, len(a.bases))
    elif a.type == ac.SOFT_CLIP:
      continue
    else:
      raise ValueError('Unexpected alt allele')
  return out


def _simplify_ref_alt(ref: str, alt: str) -> str:
  """nucleus SimplifyRefAlt: shared suffix removed (keeping one base), as "ref->alt"."""
  shortest = min(len(ref), len(alt))
  n = 0
  while n < shortest - 1 and ref[len(ref) - 1 - n] == alt[len(alt) - 1 - n]:
    n += 1
  return '%s->%s' % (ref[:len(ref) - n], alt[:len(alt) - n])


def _worth_looking_at(allele_counter, min_count: int = 0):
  """The AlleleCounts a caller has to visit: without read alleles there is no alternate allele,
  and with fewer than `min_count` reads carrying one no allele reaches the caller's count
  threshold (the device counter answers both from its event arrays)."""
  narrowed = getattr(allele_counter, 'counts_with_alt_support', None)
  if narrowed is not None and min_count > 1:
    return narrowed(min_count)
  sparse = getattr(allele_counter, 'counts_with_read_alleles', None)
  return sparse() if sparse is not None else allele_counter.counts()


class VariantCaller:
  def __init__(self, options: VariantCallerOptions):
    for name in ('min_count_snps', 'min_count_indels', 'min_fraction_snps', 'min_fraction_indels',
                 'fraction_reference_sites_to_emit'):
      if getattr(options, name) < 0:
        raise ValueError('%s must be >= 0' % name)           # CHECK_GE in the constructor
    if options.fraction_reference_sites_to_emit > 0:
      raise NotImplementedError('fraction_reference_sites_to_emit (reference-site sampling)')
    self._options = options
    self._min_fraction_f32 = (float(np.float32(options.min_fraction_indels)), float(np.float32(options.min_fraction_snps)))

  # ---- gVCF (variant_caller.py VariantCaller.reference_confidence / make_gvcfs)
  def reference_confidence(self, n_ref: int, n_total: int) -> Tuple[int, Tuple[float, float, float]]:
    """-> (raw GQ, normalised log10 likelihoods) through the cached table; deeper sites rescaled."""
    if self._options.ploidy != 2:
      raise NotImplementedError('reference confidence is restated for ploidy 2')
    if n_ref < 0 or n_total < n_ref:
      raise ValueError('Invalid read counts: n_ref=%d n_total=%d' % (n_ref, n_total))
    n_ref, n_total = rescale_read_counts_if_necessary(n_ref, n_total, self._options.max_cache_coverage)
    o = self._options
    table = reference_confidence_table(float(o.p_error), int(o.max_gq), int(o.max_cache_coverage))
    e = table[n_total * (n_total + 1) // 2 + n_ref]
    return int(e['gq']), tuple(float(x) for x in e['likelihoods'])

  def make_gvcfs(self, allele_count_summaries, include_med_dp: bool = False) -> List[T.Variant]:
    """gVCF reference blocks of one allele counter's summary counts (AlleleCounter.summary_counts
    tuples or AlleleCountSummary-like objects): consecutive sites with equal (quantised GQ,
    has_valid_gl) form one record; a non-ACGT IUPAC reference base ends a block and gets none."""
    out: List[T.Variant] = []
    group: List = []
    group_key = None

    def flush():
      if group:
        first, last = group[0], group[-1]
        depths = [g[4] for g in group]
        out.append(gvcf_record(first[0], first[1], last[1] + 1, first[2], first[5], min(g[6] for g in group),
                               min(depths), int(statistics.median(depths)) if include_med_dp else None,
                               group_key[1], self._options.sample_name))

    for s in allele_count_summaries:
      name, pos, ref_base, n_ref, n_total = _summary_fields(s)
      if ref_base in _CANONICAL:
        raw_gq, lp = self.reference_confidence(n_ref, n_total)
        key = (quantize_gq(raw_gq, self._options.gq_resolution), max(lp) == lp[0])
        row = (name, pos, ref_base, n_ref, n_total, lp, raw_gq)
      elif ref_base in _IUPAC_NON_CANONICAL:
        key, row = None, None
      else:
        raise ValueError('Invalid reference base %r at %s:%d' % (ref_base, name, pos))
      if key != group_key:
        flush()
        group, group_key = [], key
      if row is not None:
        group.append(row)
    flush()
    return out

  # ---- thresholds
  def _min_count(self, allele) -> int:
    return self._options.min_count_snps if allele.type == ac.SUBSTITUTION else self._options.min_count_indels

  def _min_fraction(self, allele) -> float:
    # VariantCallerOptions.min_fraction_* are proto `float` fields: the reference compares the double ratio
    # count / total with the threshold ROUNDED TO FLOAT32 (variant_calling_multisample.cc:250-254).  float32(0.1) is
    # above 0.1, so an allele at exactly 10 % is rejected there; comparing with the Python double would keep it
    # (found by tests/test_reference_calling_cpu.py, which runs the reference's own caller).
    return self._min_fraction_f32[allele.type == ac.SUBSTITUTION]

  def is_good_alt_allele(self, allele, total_count: int) -> bool:
    """IsGoodAltAllele (:232-238)."""
    return (allele.type not in (ac.REFERENCE, ac.SOFT_CLIP) and allele.count >= self._min_count(allele) and
            (1.0 * allele.count) / total_count >= self._min_fraction(allele))

  def select_alt_alleles(self, allele_count) -> List:
    """SelectAltAlleles (:244-258)."""
    total = ac.total_allele_counts(allele_count)
    return [a for a in ac.sum_allele_counts(allele_count) if self.is_good_alt_allele(a, total)]

  # ---- one position
  def call_variant(self, allele_count) -> Optional[T.DeepVariantCall]:
    """CallVariant (:622-671)."""
    if not allele_count.ref_base or any(b not in _CANONICAL for b in allele_count.ref_base):
      return None
    alt_alleles = self.select_alt_alleles(allele_count)
    if not alt_alleles:
      return None                              # (KeepReferenceSite is not restated)
    return self._call_with_alt_alleles(allele_count, alt_alleles, ac.total_allele_counts(allele_count))

  def _call_with_alt_alleles(self, allele_count, alt_alleles, dp: int) -> T.DeepVariantCall:
    """CallVariant behind SelectAltAlleles (:640-671); `dp` = TotalAlleleCounts(allele_count)."""
    refbases = calc_ref_bases(allele_count.ref_base, alt_alleles)
    allele_map = build_allele_map(alt_alleles, refbases)
    alternate_bases = sorted(allele_map.values())
    pos = allele_count.position
    variant = T.Variant(reference_name=pos.reference_name, start=pos.position,
                        end=pos.position + len(refbases), reference_bases=refbases,
                        alternate_bases=alternate_bases,
                        calls=[T.VariantCall(call_set_name=self._options.sample_name, genotype=[-1, -1])])
    call = T.DeepVariantCall(variant=variant)
    self._add_read_depths(allele_count, alt_alleles, allele_map, refbases, variant, dp)
    self._add_supporting_reads(allele_count.read_alleles, allele_map, refbases, call,
                               getattr(allele_count, 'read_rows', None))
    return call

  def calls_from_allele_counts(self, allele_counts: Sequence) -> List[T.DeepVariantCall]:
    out = []
    for allele_count in allele_counts:
      call = self.call_variant(allele_count)
      if call is not None:
        out.append(call)
    return out

  def _least_allele_count(self) -> int:
    return min(self._options.min_count_snps, self._options.min_count_indels)

  def candidate_options(self, positions_only: bool = False) -> CandidateOptions:
    return CandidateOptions.from_caller_options(self._options, positions_only)

  def calls_from_allele_counter(self, allele_counter) -> List[T.DeepVariantCall]:
    on_device = getattr(allele_counter, 'candidates', None)
    if on_device is not None:
      # the device selected the alleles (candidates.hip); the calls are built for its sites only
      return [self._call_with_alt_alleles(site, site.selected, site.total)
              for site in on_device(self.candidate_options())]
    return self.calls_from_allele_counts(_worth_looking_at(allele_counter, self._least_allele_count()))

  def call_positions_from_allele_counter(self, allele_counter) -> List[int]:
    on_device = getattr(allele_counter, 'candidate_positions', None)
    if on_device is not None:
      return on_device(self.candidate_options(positions_only=True))
    return self.call_positions_from_allele_counts(_worth_looking_at(allele_counter, self._least_allele_count()))

  def call_positions_from_allele_counts(self, allele_counts: Sequence) -> List[int]:
    """CallPositionsFromAlleleCounts / CallVariantPosition (variant_calling_multisample.cc:940-1004):
    the positions that WILL become candidates -- the first pass of track_ref_reads, which tells
    the allele counter where to keep the reference-supporting reads by name."""
    out = []
    for allele_count in allele_counts:
      if not allele_count.ref_base or any(b not in _CANONICAL for b in allele_count.ref_base):
        continue
      if self.select_alt_alleles(allele_count):
        out.append(allele_count.position.position)
    return out

  # ---- annotations
  def _add_read_depths(self, allele_count, alt_alleles, allele_map, refbases, variant, dp=None):
    """AddReadDepths (:298-351): DP, AD, VAF on the first call."""
    info = variant.calls[0].info
    if dp is None:
      dp = ac.total_allele_counts(allele_count)
    info['DP'] = T.ListValue(values=[T.Value(int_value=dp)])
    by_simplified = {}
    counts = {_allele_order(a): a.count for a in alt_alleles}
    for key, alt in allele_map.items():
      by_simplified[_simplify_ref_alt(refbases, alt)] = counts[key]
    if len(by_simplified) != len(allele_map):
      raise ValueError('Non-unique alternative alleles!')
    ad = [allele_count.ref_supporting_read_count]
    vaf = []
    for alt in variant.alternate_bases:
      n = by_simplified.get(_simplify_ref_alt(variant.reference_bases, alt), 0)
      ad.append(n)
      vaf.append(1.0 * n / dp if dp > 0 else 0.0)
    info['AD'] = T.ListValue(values=[T.Value(int_value=v) for v in ad])
    info['VAF'] = T.ListValue(values=[T.Value(number_value=v) for v in vaf])

  def _add_supporting_reads(self, read_alleles, allele_map, refbases, call, read_rows=None):
    """AddSupportingReads (:673-713).  `read_rows` (a device caller's site: the table row behind every entry of
    read_alleles) fills call.support_rows next to allele_support: the same keys, the same order, the same suffix."""
    suffix = ''
    if len(call.variant.reference_bases) > len(refbases):
      suffix = call.variant.reference_bases[len(refbases):]
    rows = {} if read_rows is not None else None
    for read_name, allele in read_alleles.items():
      if allele.type != ac.REFERENCE:
        alt = allele_map.get(_allele_order(allele))
        key = K_SUPPORTING_UNCALLED_ALLELE if alt is None else alt + suffix
        call.allele_support.setdefault(key, T.SupportingReads()).read_names.append(read_name)
        if rows is not None:
          rows.setdefault(key, []).append(read_rows[read_name])
        call.allele_support_ext.setdefault(key, []).append(T.ReadSupport(read_name, bool(allele.is_low_quality)))
      elif self._options.track_ref_reads:
        # REFERENCE read alleles are kept by name only under track_ref_reads, at candidate
        # positions (variant_calling.cc:706, variant_calling_multisample.cc:1231-1247)
        call.ref_support.append(read_name)
        call.ref_support_ext.append(T.ReadSupport(read_name, bool(allele.is_low_quality)))
    if rows is not None:
      call.support_rows = {key: np.array(r, np.int64) for key, r in rows.items()}
