"""The cases of the genotype merge shared by test_genotype_cpu.py and
test_hip_genotype.py, and a plain-Python restatement of the contract, dict-of-lists, that shares no code with the
product: the host code is checked against it, the device against the host code.

A case is (probs float32 [N, 3], sites [(n_alts, [the alt indices of each item])], t).  `t` is step 2's threshold as
the native entry points take it; T1 is its value for the default --qual_filter 1.0.
"""
import math

import numpy as np

T1 = 0.20567175613067676          # dv_genotype_min_nonref_prob(1.0); test_genotype_cpu.py checks the figure
DEVICE_MAX_ALTS = 6
F0, F1, F1E10 = np.float32(0), np.float32(1), np.float32(1e10)


def f32(rows):
  return np.array(rows, np.float32).reshape(-1, 3)


def sums_to_one(p):
  total = (p[:, 0] + p[:, 1]) + p[:, 2]
  return np.abs(total - F1) <= np.float32(1e-6)


def seeded_rows(n, seed, alpha=1.0):
  """n float32 Dirichlet(alpha, alpha, alpha) rows whose float32 sum is within 1e-6 of one."""
  rng = np.random.default_rng(seed)
  rows = np.zeros((0, 3), np.float32)
  while rows.shape[0] < n:
    p = rng.dirichlet([alpha] * 3, 2 * n).astype(np.float32)
    rows = np.concatenate([rows, p[sums_to_one(p)]])
  return np.ascontiguousarray(rows[:n])


def combinations(n_alts):
  """alt_allele_combinations: every single alt, then every pair."""
  return [[a] for a in range(n_alts)] + [[a, b] for a in range(n_alts) for b in range(a + 1, n_alts)]


# ------------------------------------------------------------------------------------------ the restatement
def round_row(p, already_rounded=False):
  """Step 1 on one float32 row -> ([three Python floats], the sum is off)."""
  p = [np.float32(x) for x in p]
  if already_rounded:
    return [float(x) for x in p], bool(np.abs((p[0] + p[1]) + p[2] - F1) > np.float32(1e-6))
  r = [np.rint(x * F1E10) / F1E10 for x in p]
  lowest = 0
  for k in (1, 2):
    if p[k] < p[lowest]:
      lowest = k
  rest = F0
  for k in range(3):
    rest = rest + (F0 if k == lowest else r[k])
  r[lowest] = max(F0, np.rint((F1 - rest) * F1E10) / F1E10)
  assert all(x.dtype == np.float32 for x in r)
  bad = bool(np.abs((p[0] + p[1]) + p[2] - F1) > np.float32(1e-6))
  return [float(x) for x in r], bad


def reference(probs, sites, t, already_rounded=False):
  """-> dict(rounded, pred_off, predictions, best, removed, status), lists in the native arrays' layout."""
  out = dict(rounded=[], pred_off=[0], predictions=[], best=[], removed=[], status=[])
  i = 0
  for n_alts, items in sites:
    rows, bad = [], False
    for alts in items:
      r, off = round_row(probs[i], already_rounded)
      i += 1
      bad = bad or off
      rows.append((tuple(alts), r))
      out['rounded'].append(r)
    removed = set()
    if len(items) > 1 and t > 0:
      singles = {}
      for alts, r in rows:
        if len(alts) == 1:
          singles.setdefault(alts[0], []).append(min(r[1] + r[2], 1.0))
      s = {a: max(v) for a, v in singles.items()}
      removed = {a for a in s if s[a] < t}
      if len(removed) == n_alts:
        stays = 0
        for a in range(1, n_alts):
          if s[a] > s[stays]:
            stays = a
        removed.discard(stays)
    kept = [a for a in range(n_alts) if a not in removed]
    allele = {a: k + 1 for k, a in enumerate(kept)}
    contributions = {}
    for alts, r in rows:
      if any(a in removed for a in alts):
        continue
      named = sorted(allele[a] for a in alts)
      contributions.setdefault((0, 0), []).append(r[0])
      for a in named:
        contributions.setdefault((0, a), []).append(r[1])
      for k, a in enumerate(named):
        for b in named[k:]:
          contributions.setdefault((a, b), []).append(r[2])
    order = [(a, b) for b in range(len(kept) + 1) for a in range(b + 1)]      # VCF order
    incomplete = any(g not in contributions for g in order)
    predictions = [min(contributions[g]) if g in contributions else math.inf for g in order]
    best = -1
    if not incomplete:
      if len(items) != 1:
        total = sum(predictions)
        predictions = [p / total for p in predictions]
      best = predictions.index(max(predictions))
    slots = (n_alts + 1) * (n_alts + 2) // 2
    out['predictions'].extend(predictions + [0.0] * (slots - len(predictions)))
    out['pred_off'].append(out['pred_off'][-1] + slots)
    out['best'].append(best)
    out['removed'].append(sum(1 << a for a in removed))
    out['status'].append(1 if bad else 2 if incomplete else 0)
  return out


def single_alt_score(row):
  r, _ = round_row(row)
  return min(r[1] + r[2], 1.0)


# ------------------------------------------------------------------------------------------ the cases
def _first_clamping_row():
  """A seeded row whose rounded rest exceeds one: the residual 1 - rest is negative and clamps to 0."""
  for p in seeded_rows(256, 11, 0.05):
    lowest = int(np.argmin(p))
    r = [np.rint(x * F1E10) / F1E10 for x in p]
    rest = F0
    for k in range(3):
      rest = rest + (F0 if k == lowest else r[k])
    if rest > F1:
      return p
  raise AssertionError('no clamping row among 256')


def hand_made_rows():
  """name -> one float32 row."""
  tiny, tinier = np.float32(1.23456789e-4), np.float32(5.4321e-5)      # the second is the row's minimum
  return {
      'tie_0_1': f32([0.25, 0.25, 0.5])[0],
      'tie_1_2': f32([0.5, 0.25, 0.25])[0],
      'tie_0_2': f32([0.25, 0.5, 0.25])[0],
      'one_zero_zero': f32([1, 0, 0])[0],
      'below_1e-3': np.array([F1 - tiny - tinier, tiny, tinier], np.float32),
      'clamps': _first_clamping_row(),
      'bad_sum': np.array([0.5, 0.25, np.float32(0.25) + np.float32(2e-6)], np.float32),
  }


def mixed_call(n_sites, seed):
  """n_sites sites with 1..3 alts in a seeded mix, complete: output slices start at irregular offsets."""
  rng = np.random.default_rng(seed)
  sites = [(int(a), combinations(int(a))) for a in rng.integers(1, 4, n_sites)]
  n_items = sum(len(items) for _, items in sites)
  return seeded_rows(n_items, seed + 1, 0.4), sites, T1


def cases():
  """name -> (probs, sites, t)."""
  low0, low1 = [.9, .06, .04], [.85, .1, .05]          # single-alt scores .1 and .15, both below T1
  c = {}
  c['a1'] = (f32([[.1, .7, .2]]), [(1, [[0]])], T1)
  c['a2_complete'] = (f32([[.2, .5, .3], [.3, .4, .3], [.1, .2, .7]]), [(2, combinations(2))], T1)
  c['a2_alt0_removed'] = (f32([low0, [.2, .5, .3], [.5, .3, .2]]), [(2, combinations(2))], T1)
  c['a2_alt1_removed'] = (f32([[.2, .5, .3], low0, [.5, .3, .2]]), [(2, combinations(2))], T1)
  c['a2_both_below_best_stays'] = (f32([low0, low1, [.5, .3, .2]]), [(2, combinations(2))], T1)
  c['a2_both_below_tie_first_stays'] = (f32([low0, low0, [.5, .3, .2]]), [(2, combinations(2))], T1)
  c['a3'] = (seeded_rows(6, 3), [(3, combinations(3))], T1)
  c['a3_low'] = (seeded_rows(6, 4, 0.2), [(3, combinations(3))], T1)
  c['a6'] = (seeded_rows(21, 5), [(6, combinations(6))], T1)
  c['a6_low'] = (seeded_rows(21, 6, 0.2), [(6, combinations(6))], T1)
  c['a7'] = (seeded_rows(28, 7), [(7, combinations(7))], T1)
  c['a7_low_between_small_sites'] = (
      np.concatenate([seeded_rows(1, 8), seeded_rows(28, 9, 0.2), seeded_rows(3, 10)]),
      [(1, [[0]]), (7, combinations(7)), (2, combinations(2))], T1)
  order = [4, 0, 5, 2, 1, 3]
  c['a3_shuffled'] = (np.ascontiguousarray(c['a3'][0][order]), [(3, [combinations(3)[k] for k in order])], T1)
  c['a2_singles_only_incomplete'] = (f32([[.2, .5, .3], [.3, .4, .3]]), [(2, [[0], [1]])], T1)
  c['a2_no_items_incomplete'] = (f32([[.2, .5, .3]]), [(2, []), (1, [[0]])], T1)
  base = c['a2_complete'][0]
  s1 = single_alt_score(base[1])                       # alt 1's score, the smaller of the two
  c['a2_s_equals_t'] = (base, [(2, combinations(2))], s1)
  c['a2_s_just_below_t'] = (base, [(2, combinations(2))], float(np.nextafter(s1, 2.0)))
  c['a2_qual_filter_0'] = (c['a2_alt0_removed'][0], [(2, combinations(2))], 0.0)
  c['zero_sites'] = (np.zeros((0, 3), np.float32), [], T1)
  rows = hand_made_rows()
  c['hand_made_rows'] = (np.stack(list(rows.values())), [(1, [[0]])] * len(rows), T1)
  c['bad_sum_in_a2'] = (np.stack([base[0], rows['bad_sum'], base[2]]), [(2, combinations(2))], T1)
  c['dirichlet_4096'] = (seeded_rows(4096, 12, 0.05), [(1, [[0]])] * 4096, T1)
  for n in (1, 63, 64, 65, 257):
    c['mixed_%d' % n] = mixed_call(n, 100 + n)
  return c


def above_device_limit(sites):
  return sum(1 for n_alts, items in sites if n_alts > DEVICE_MAX_ALTS or len(items) > 21)
