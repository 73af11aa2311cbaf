"""What the device window pass (dv_select_windows_batch, deepvariant_amd/csrc/window_select.hip) is held against,
shared by tests/test_hip_window_select.py: the expected answers always come from the host functions of
deepvariant_amd/realigner/window_selector.py on a separately run plain counter, never from the device pass."""
import copy

import numpy as np

from deepvariant_amd import allelecounter as A
from deepvariant_amd import dv_types as T
from deepvariant_amd.realigner import realigner as R
from deepvariant_amd.realigner import window_selector as ws


def linear_config(distance=None, **model):
  """The realigner's default model (ws_use_window_selector_model=True): ALLELE_COUNT_LINEAR."""
  config = copy.deepcopy(R.realigner_config(ws_use_window_selector_model=True).ws_config)
  assert config.window_selector_model.model_type == ws.ALLELE_COUNT_LINEAR
  if distance is not None:
    config.min_windows_distance = distance
  for name, value in model.items():
    setattr(config.window_selector_model.allele_count_linear_model, name, value)
  return config


def threshold_config(distance=None, strict=False, min_allele_support=None, lo=None, hi=None):
  """The realigner's VARIANT_READS model (ws_use_window_selector_model=False)."""
  config = copy.deepcopy(R.realigner_config(ws_use_window_selector_model=False).ws_config)
  assert config.window_selector_model.model_type == ws.VARIANT_READS
  if distance is not None:
    config.min_windows_distance = distance
  config.enable_strict_insertion_filter = strict
  if min_allele_support is not None:
    config.min_allele_support = min_allele_support
  if lo is not None:
    config.window_selector_model.variant_reads_model.min_num_supporting_reads = lo
  if hi is not None:
    config.window_selector_model.variant_reads_model.max_num_supporting_reads = hi
  return config


def interval(counter):
  return T.Range(counter._contig, counter.interval_start(), counter.interval_start() + counter.interval_length())   # pylint: disable=protected-access


def host_scores(config, counter):
  """The per-position figures the host's decision is taken on, as uint32 words: the float32 scores' bit patterns,
  or the VARIANT_READS counts."""
  if config.window_selector_model.model_type == ws.ALLELE_COUNT_LINEAR:
    scores = ws.allele_count_linear_candidates_from_allele_counter(
        counter, config.window_selector_model.allele_count_linear_model)
    return np.asarray(scores, np.float32).view(np.uint32)
  return np.asarray(ws.variant_reads_candidates_from_allele_counter(counter, config), np.int32).view(np.uint32)


def host_answer(config, counter):
  """-> (candidate mask, [(start, end)], scores as uint32) from a counter that has counted on its own."""
  expanded = interval(counter)
  positions = ws._candidates_from_counter(config, counter, expanded)              # pylint: disable=protected-access
  mask = np.zeros(counter.interval_length(), bool)
  mask[np.asarray([p - expanded.start for p in positions], np.int64)] = True
  windows = ws._candidates_to_windows(config, positions, expanded.reference_name)  # pylint: disable=protected-access
  return mask, [(w.start, w.end) for w in windows], host_scores(config, counter)


def device_answer(config, counter):
  starts, ends, mask, scores = counter.windows(config, want_debug=True)
  return mask, list(zip(starts.tolist(), ends.tolist())), scores


def check(make, config, scores_too=True):
  """`make()` -> fresh counters of one batch.  The batch's device answers (mask, windows, scores bit for bit) against
  the host's on separately counted plain counters; and a windows-only pass brings the same windows and leaves the
  counters uncounted.  -> the host answers."""
  plain = make()
  A.AlleleCounter.run_batch(plain)
  want = [host_answer(config, c) for c in plain]
  device = make()
  fresh = [c._events is None for c in device]                                     # pylint: disable=protected-access
  A.AlleleCounter.run_batch(device, windows=config, window_debug=True)
  bare = make()
  A.AlleleCounter.run_batch(bare, windows=config)
  for k, (c, b, (mask, windows, scores)) in enumerate(zip(device, bare, want)):
    got_mask, got_windows, got_scores = device_answer(config, c)
    assert np.array_equal(got_mask, mask), (k, np.nonzero(got_mask != mask)[0][:10])
    assert got_windows == windows, k
    if scores_too:
      assert np.array_equal(got_scores, scores), (k, np.nonzero(got_scores != scores)[0][:10])
    starts, ends = b.windows(config)
    assert list(zip(starts.tolist(), ends.tolist())) == windows, k
    if fresh[k]:
      assert c._events is None and b._events is None                              # pylint: disable=protected-access
  return want


def order_free_scores(counter, model):
  """The linear model's scores summed without an order: every term in float64 (the float32 coefficients and
  reference terms are exact there, and so are their sums at these depths), rounded to float32 once."""
  f32 = np.float32
  coeff = {A.SUBSTITUTION: f32(model.coeff_substitution), A.SOFT_CLIP: f32(model.coeff_soft_clip),
           A.INSERTION: f32(model.coeff_insertion), A.DELETION: f32(model.coeff_deletion),
           A.REFERENCE: f32(model.coeff_reference)}
  n = counter.interval_length()
  ref_terms = np.asarray(counter.ref_supporting_read_counts()).astype(np.float32) * f32(model.coeff_reference)
  total = np.full(n, np.float64(f32(model.bias))) + ref_terms.astype(np.float64)
  for i, ac in ws._positions_with_read_alleles(counter):                          # pylint: disable=protected-access
    for allele in ac.read_alleles.values():
      m = len(allele.bases)
      if allele.type in (A.SUBSTITUTION, A.REFERENCE):
        lo, hi = i, i + 1
      elif allele.type in (A.SOFT_CLIP, A.INSERTION):
        lo, hi = i + 1 - (m - 1), i + m
      else:
        lo, hi = i + 1, i + m
      total[max(lo, 0):min(hi, n)] += np.float64(coeff[allele.type])
  return total.astype(np.float32)
