"""Inputs shared by test_fast_pass_batch_abi_cpu.py and test_hip_fast_pass.py: a direct transcription of the fast
pass's closed form (include/dvhip.h, "the fast pass over many windows in one call"), the hand-made windows and the
seeded ones.  A window is what fast_pass_aligner.fast_pass_batch takes, plus `options` and a `name`."""
import numpy as np

MATCH, MISMATCH = 4, 6      # the class defaults
DEFAULT_M = 2               # max_num_of_mismatches = 0 keeps it: dv_aligner_options has no way to ask for 0


def closed_form(reads, haplotype, reference, prefix, suffix, k, max_mismatches, match=MATCH, mismatch=MISMATCH):
  """-> (score, discarded, [(position, score)], [(key, start, mismatches, score) of every accepted start per read])."""
  n = len(haplotype)
  covered = [False] * n
  where = {}
  for i in range(n - k + 1):
    where.setdefault(haplotype[i:i + k], []).append(i)
  index = {r.upper()[off:off + k] for r in reads if len(r) > k for off in range(len(r) - k + 1)}
  rows, accepted = [], []
  for read in reads:
    read, best, mine = read.upper(), None, []
    size = len(read)
    if k < size <= n:
      keys = {}
      for off in range(size - k + 1):
        for i in where.get(read[off:off + k], ()):            # every seed (i, off)
          s = max(0, i - off)
          if s + size <= n:
            keys[s] = min(keys.get(s, (i, off)), (i, off))
      for s, key in keys.items():
        mm = sum(1 for p in range(size) if haplotype[s + p] != read[p] and 'N' not in (haplotype[s + p], read[p]))
        if mm > max_mismatches:
          continue
        covered[key[0]:s + size] = [True] * (s + size - key[0])
        score = (size - mm) * match - mm * mismatch
        mine.append((key, s, mm, score))
        if score > 0 and (best is None or (-score, key) < (-best[0], best[1])):
          best = (score, key, s)
    rows.append((best[2], best[0]) if best else (-1, 0))
    accepted.append(mine)
  end = n if suffix > n else n - suffix          # the host's unsigned n - suffix wraps
  discarded = haplotype != reference and any(
      not covered[i] and haplotype[i:i + k] in index for i in range(n - k + 1) if prefix <= i < end)
  total = 0 if discarded else sum(s for _, s in rows)
  if total == 0:
    rows = [(-1, 0)] * len(reads)
  return total, discarded, rows, accepted


def window_model(w):
  """closed_form for every haplotype of a window -> what fast_pass_batch returns for it, as lists."""
  o = w.get('options', {})
  out = dict(haplotype_score=[], haplotype_discarded=[], read_position=[], read_score=[])
  for h in w['haplotypes']:
    total, discarded, rows, _ = closed_form(w['reads'], h, w.get('reference'), w.get('ref_prefix_len', 0),
                                            w.get('ref_suffix_len', 0), o.get('kmer_size', 32),
                                            o.get('max_num_of_mismatches', 0) or DEFAULT_M, o.get('match', 0) or MATCH,
                                            o.get('mismatch', 0) or MISMATCH)
    out['haplotype_score'].append(total)
    out['haplotype_discarded'].append(int(discarded))
    out['read_position'].append([p for p, _ in rows])
    out['read_score'].append([s for _, s in rows])
  return out


def _w(name, reads, haplotypes, k, reference=None, prefix=0, suffix=0, expect_discarded=None, **options):
  return dict(name=name, reads=list(reads), haplotypes=list(haplotypes), reference=reference, ref_prefix_len=prefix,
              ref_suffix_len=suffix, expect_discarded=expect_discarded, options=dict(kmer_size=k, **options))


def _dna(rng, n, letters='ACGT'):
  return ''.join(rng.choice(list(letters), size=n))


def _mutate(s, positions):
  swap = {'A': 'C', 'C': 'G', 'G': 'T', 'T': 'A', 'N': 'A'}
  return ''.join(swap[c] if p in positions else c for p, c in enumerate(s))


#                  0         1         2         3         4
#                  0123456789012345678901234567890123456789012
COVER = 'TTGACCATGCAAGTCGGATACCTGAACGTTCAGGCATTAGCCA'       # 43 bytes, no repeated 4-mer


def hand_made():
  rng = np.random.default_rng(20)
  cases = []
  # -- start 0 through a negative diagonal, k = 3: ACGACTGA against ACTACGGA... mismatches at 2 and 5, so diagonal 0
  # holds no run of 3; the seed is H[0:3] = ACT = R[3:6], which the host's clamp turns into start 0
  hap = 'ACTACGGATTCC'
  cases.append(_w('negative diagonal accepted at 0', ['ACGACTGA'], [hap], 3, reference=hap))
  # the same seed, but start 0 is past M = 1 while the copy at 12 is exact
  hap = 'ACTACGGATTCCACGACTGATT'
  cases.append(_w('negative diagonal rejected at 0, later start accepted', ['ACGACTGA'], [hap], 3, reference=hap,
                  max_num_of_mismatches=1))
  # -- equal best scores in a tandem repeat: starts 0, 3, 6, 9 are all exact; start 0's key (0, 0) is the smallest
  cases.append(_w('tandem repeat tie', ['ACGACGACG', 'CGACGAC'], ['ACGACGACGACGACGACG'], 3, reference='ACGACGACGACGACGACG'))
  # the tie that start 0 reaches through a negative diagonal, k = 5: one mismatch at start 0 and at start 6; the
  # negative diagonal -6 gives H[0:5] = R[6:11], key (0, 6), ahead of start 6's key (11, 5)
  hap = 'GACCGAGACCGAGACCGAGACTT'
  cases.append(_w('tie reached through a negative diagonal', ['GACCTAGACCGAGAC'], [hap], 5, reference=hap,
                  max_num_of_mismatches=1))
  # -- N: equal to N inside a seed, a wildcard in the mismatch count
  cases.append(_w('N in seeds and as wildcard',
                  ['ACNGTCA', 'ANNGTNA', 'ACNNNCATG', 'TCNGACC', 'NNNNNNN', 'GTCANGC'],
                  ['ACNGTCATGCNNGTCATGC', 'ACAGTCATGCNNNNNNNAC'], 3, max_num_of_mismatches=1))
  # -- exactly M and M + 1 mismatches (dv_aligner_options cannot ask for M = 0: the value 0 keeps the default, 2)
  base = _dna(rng, 60)
  for m in (1, 2):
    reads = []
    for count in (m, m + 1):
      for start in (0, 11, 30):
        piece = base[start:start + 30]
        reads.append(_mutate(piece, set(range(8, 8 + 4 * count, 4))))
    cases.append(_w('M = %d: M and M + 1 mismatches' % m, reads, [base], 8, max_num_of_mismatches=m))
  # -- an accepted start with score <= 0 marks coverage but places no read
  hap = COVER[:30]
  # (the second read: 21 - 25 < 0 with one mismatch): without it 12..13 would be a hole, see the third haplotype's M
  cases.append(_w('accepted with score <= 0', [hap[:12], _mutate(hap[8:30], {9}), hap[14:30]], [hap], 4,
                  reference='', match=1, mismatch=25, max_num_of_mismatches=1, expect_discarded=[0]))
  cases.append(_w('the same read rejected: the hole it covered', [hap[:12], _mutate(hap[8:30], {9, 15}), hap[14:30]],
                  [hap], 4, reference='', match=1, mismatch=25, max_num_of_mismatches=1, expect_discarded=[1]))
  # -- read lengths around k and n
  hap = COVER[:24]
  cases.append(_w('L = k, k + 1, n, n + 1 and a read that ends at n',
                  [hap[3:9], hap[3:10], hap, hap + 'A', hap[10:24], hap[:5], 'ACG', ''], [hap], 6))
  # -- coverage holes.  The host looks at a position's coverage only where its k-mer is in the index: the probe
  # brings the k-mers at 28, 29 and 30 but is itself accepted nowhere
  probe = 'GGGG' + COVER[28:34] + 'TTTT'
  reads = [COVER[0:16], COVER[12:28], COVER[31:43], probe]          # nothing covers 28, 29, 30
  cases.append(_w('a hole discards', reads, [COVER], 4, reference='', expect_discarded=[1]))
  cases.append(_w('the hole, but its k-mers are in no read', reads[:3], [COVER], 4, reference='', expect_discarded=[0]))
  cases.append(_w('the same hole inside the prefix', reads, [COVER], 4, reference='', prefix=31, expect_discarded=[0]))
  cases.append(_w('the same hole inside the suffix', reads, [COVER], 4, reference='', suffix=15, expect_discarded=[0]))
  cases.append(_w('the hole one past the prefix and the suffix', reads, [COVER, COVER], 4, reference='', prefix=30,
                  suffix=12, expect_discarded=[1, 1]))
  cases.append(_w('the same hole on the reference haplotype', reads, [COVER, COVER[:42] + 'C'], 4, reference=COVER,
                  expect_discarded=[0, 1]))
  cases.append(_w('no reference at all', reads, [COVER], 4, reference=None, expect_discarded=[1]))
  # the host's unsigned n - suffix wraps: nothing is excluded; the probe does not fit at 24 but is in the index
  cases.append(_w('a suffix longer than the haplotype', reads[:2] + [probe], [COVER[:34]], 4, reference='', suffix=40,
                  expect_discarded=[1]))
  # -- an accepted alignment that is not its read's best closes the hole: COVER[0:12] is exact at 0 and has one
  # mismatch at 24, where nothing else covers 24..32; with three mismatches there it is rejected and the hole stays
  q = COVER[0:12]
  closed = COVER[:24] + _mutate(q, {5}) + COVER[36:]
  still_open = COVER[:24] + _mutate(q, {5, 7, 9}) + COVER[36:]
  cases.append(_w('a second-best alignment closes the hole', [COVER[0:16], COVER[10:24], closed[33:43], q],
                  [closed, still_open], 4, reference='', expect_discarded=[0, 1]))
  # -- lower case and bytes outside ACGTN
  cases.append(_w('lower-case reads', [COVER[2:20].lower(), COVER[18:43].swapcase(), 'ttgaccatgcnagt'], [COVER], 4))
  odd = 'ACGRYACG-TTKACGA*CGTAC'
  cases.append(_w('bytes outside ACGTN', [odd[2:12], odd[8:20].lower(), 'ACGRTACG', odd[10:]], [odd, odd.lower()], 3))
  # -- diagonal counts around the wave width: n - L + 1 diagonals for the 20-byte reads
  for count in (63, 64, 65, 127, 128, 129):
    hap = _dna(rng, count + 19)
    starts = sorted({0, 1, 62, 63, 64, count - 2, count - 1} & set(range(count)))
    reads = [hap[s:s + 20] for s in starts] + [_mutate(hap[count - 1:count + 19], {0, 19})]
    cases.append(_w('%d diagonals' % count, reads, [hap], 6, reference=hap))
  # -- more reads than the workgroup has waves; one read
  hap = _dna(rng, 90)
  cases.append(_w('eleven reads', [hap[s:s + 25] for s in range(0, 66, 6)], [hap, _mutate(hap, {40})], 7))
  cases.append(_w('one read', [hap[30:70]], [hap, hap[:69], hap[31:]], 7))
  cases.append(_w('no reads', [], [hap], 7))
  cases.append(_w('no haplotypes', [hap[:30]], [], 7))
  cases.append(_w('an empty haplotype', [hap[:30]], ['', hap], 7, reference=''))
  return cases


def over_the_cap(cap):
  """A haplotype one byte over the device cap beside one exactly at it, reads placed at both ends."""
  rng = np.random.default_rng(21)
  hap = _dna(rng, cap + 1)
  reads = [hap[0:40], hap[cap - 39:cap + 1], hap[cap - 40:cap], _mutate(hap[4000:4040], {7}), hap[100:140].lower()]
  return _w('one byte over the cap', reads, [hap, hap[:cap]], 8, reference=hap)


def seeded(seed, n_windows, small=False):
  """Windows as the realigner meets them, scaled down: a reference, 2-5 haplotypes that differ from it by a few
  substitutions and indels, 20-70 reads (small: 3-12) cut from the haplotypes with errors, some N, some lower case.
  Every window of a call shares its options."""
  rng = np.random.default_rng(seed)
  out = []
  k = int(rng.integers(3, 9))          # one set of options per call
  options = dict(max_num_of_mismatches=int(rng.integers(0, 3)), match=int(rng.choice([0, 1, 4])),
                 mismatch=int(rng.choice([0, 2, 6, 30])))
  for w in range(n_windows):
    n = int(rng.integers(30, 90)) if small else int(rng.integers(150, 400))
    letters = 'ACGT' if rng.random() < 0.7 else 'AC'
    reference = _dna(rng, n, letters)
    haplotypes = [reference] if rng.random() < 0.8 else []
    for _ in range(int(rng.integers(2, 6)) - len(haplotypes)):
      h = list(reference)
      for _ in range(int(rng.integers(1, 4))):
        at = int(rng.integers(0, len(h)))
        kind = int(rng.integers(0, 3))
        if kind == 0:
          h[at] = str(rng.choice(list('ACGTN')))
        elif kind == 1:
          h[at:at] = list(_dna(rng, int(rng.integers(1, 6)), letters))
        else:
          del h[at:at + int(rng.integers(1, 6))]
      haplotypes.append(''.join(h))
    reads = []
    for _ in range(int(rng.integers(3, 13)) if small else int(rng.integers(20, 71))):
      h = haplotypes[int(rng.integers(0, len(haplotypes)))]
      size = int(rng.integers(4, 41)) if small else int(rng.integers(30, 120))
      at = int(rng.integers(0, max(1, len(h) - size + 1)))
      r = list(h[at:at + size])
      for _ in range(int(rng.integers(0, 4))):
        r[int(rng.integers(0, len(r)))] = str(rng.choice(list('ACGTN')))
      r = ''.join(r)
      reads.append(r.lower() if rng.random() < 0.1 else r)
    pad = int(rng.integers(0, 12))
    out.append(_w('seed %d window %d' % (seed, w), reads, haplotypes, k, reference=reference, prefix=pad,
                  suffix=int(rng.integers(0, 12)), **options))
  return out
