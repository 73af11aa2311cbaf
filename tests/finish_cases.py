"""Windows for the finish step of the realigner's alignments (csrc/realign_finish.h / .hip): hand-made ones named for
what they hold, and seeded ones from the generator idea of tools/realign_finish_check.cpp.  No GPU needed.  A case is
dict(name, windows=[...], options={...}); a window is what fast_pass_aligner.align_windows_batch takes.  Sizes are
small: references <= 400 bases, <= 40 haplotypes (96 where stated), reads <= 250 bases."""
import random

OPTIONS = dict(kmer_size=12, read_size=60)


def _bases(rng, n):
  return ''.join(rng.choice('ACGT') for _ in range(n))


def _flip(s, *at):
  s = list(s)
  for i in at:
    s[i] = 'A' if s[i] != 'A' else 'C'
  return ''.join(s)


_RNG = random.Random(20260101)
REF = _bases(_RNG, 240)
INS = REF[:120] + 'GATTTC' + REF[120:]              # an insertion of 6 behind reference base 120
DEL = REF[:120] + REF[127:]                         # a deletion of 7
BOTH = REF[:80] + 'TTGCA' + REF[80:150] + REF[154:]    # an insertion of 5 and a deletion of 4
D2 = REF[:120] + REF[122:]                          # a deletion of 2
D3 = REF[:120] + REF[123:]
I3 = REF[:120] + 'CAT' + REF[120:]
I1 = REF[:120] + ('G' if REF[120] != 'G' else 'T') + REF[120:]
CLIPPED = 'TTTTTTTTTT' + REF[10:]                   # its own alignment starts with a soft clip


def _unplaced(read):
  """Three substitutions spread over the read: past max_num_of_mismatches, so Smith-Waterman places it."""
  n = len(read)
  return _flip(read, n // 6, n // 2, n - n // 6)


def window(name, haplotypes, reads, **kw):
  """ref_prefix_len past every haplotype: the fast pass discards none for a position no read covers."""
  return dict(name=name, haplotypes=list(haplotypes), reads=list(reads), reference=kw.pop('reference', REF),
              ref_start=kw.pop('ref_start', 5000), ref_prefix_len=kw.pop('ref_prefix_len', 400), **kw)


def case(name, windows, **options):
  return dict(name=name, windows=windows if isinstance(windows, list) else [windows], options=dict(OPTIONS, **options))


def tied_window(n):
  """n - 1 haplotypes with one haplotype_score and the reference below them.  The first n // 2 carry an insertion
  of GATTTC behind base 120, the others four substitutions there (GATT), each told from its kin by a substitution
  past base 200 that no read reaches.  Read 0 ends inside the insertion and fits both kinds without a mismatch, so it
  goes to the tied haplotype the sorted walk reaches last: `49M5I` on the first kind, another CIGAR on the second.  With 17 and
  40 haplotypes std::sort leaves haplotype 1 and 19 last (the first kind), index order 15 and 38 (the second)."""
  haps = [_flip(INS if h < n // 2 else REF[:120] + 'GATT' + REF[124:], 200 + h) for h in range(n - 1)] + [REF]
  return window('tied_scores_%d_haplotypes' % n, haps, [REF[70:120] + 'GATT', REF[10:70]])


def hand_made():
  out = []
  one = lambda name, haps, reads, **opt: out.append(case(name, window(name, haps, reads), **opt))   # noqa: E731
  one('fast_pass_read_on_haplotype_with_insertion', [REF, INS], [INS[90:150], REF[10:70]])
  one('fast_pass_read_on_haplotype_with_deletion', [REF, DEL], [DEL[90:150], REF[10:70]])
  one('fast_pass_read_on_haplotype_with_both', [REF, BOTH], [BOTH[60:180], REF[10:70]], read_size=120)
  one('cigar_longer_than_the_first_download', [REF, BOTH], [BOTH[60:180]], read_size=120)   # 5 words for 1 read
  one('read_starts_inside_the_haplotypes_insertion', [REF, INS], [INS[90:150], INS[123:183]])
  one('read_starts_right_behind_the_deletion', [REF, DEL], [DEL[90:150], DEL[120:180]])
  # a read with its own insertion where the haplotype has a deletion, and the reverse
  one('read_i3_on_haplotype_d2', [REF, D2], [D2[90:150], _unplaced(D2[80:120] + 'CAT' + D2[120:160])], normalize_reads=1)
  one('read_i1_on_haplotype_d3', [REF, D3], [D3[90:150], _unplaced(D3[80:120] + 'G' + D3[120:160])])
  one('read_d2_on_haplotype_i3', [REF, I3], [I3[90:150], _unplaced(I3[80:121] + I3[123:165])], normalize_reads=1)
  one('read_d3_on_haplotype_i1', [REF, I1], [I1[90:150], _unplaced(I1[80:119] + I1[122:165])])
  one('leading_soft_clip', [REF, INS], [INS[90:150], 'GGGGGGGG' + _unplaced(INS[100:160])])
  one('soft_clipped_tail_past_the_haplotype_end', [REF, INS], [INS[90:150], _unplaced(INS[-50:]) + 'ACGTACGTAC'])
  one('read_runs_past_the_haplotype_is_cleared', [REF, INS], [INS[90:150], _unplaced(INS[-40:]) + INS[:25]])
  one('haplotype_with_soft_clips_offset_negative', [CLIPPED, INS], [CLIPPED[:60], CLIPPED[2:62], INS[90:150]])
  one('haplotype_all_n_cannot_be_aligned', [REF, 'N' * 240], [REF[10:70], 'N' * 60, REF[100:160]])
  one('equal_scores_on_reference_and_non_reference', [REF, INS], [REF[10:70], INS[90:150], REF[130:190]])
  one('equal_scores_on_two_non_reference_haplotypes', [INS, _flip(INS, 230), REF],
      [INS[90:150], INS[100:160], REF[10:70]])
  for n in (17, 40):
    out.append(case('tied_scores_%d_haplotypes' % n, tied_window(n)))
  # what is left of the read's insertion behind the haplotype's deletion could shift left: kept only under normalize_reads
  for normalize in (0, 1):
    one('non_normalized_indel_normalize_reads_%d' % normalize, [REF, D2],
        [D2[90:150], _unplaced(D2[80:120] + 'CAT' + D2[120:160])], normalize_reads=normalize)
  one('force_alignment_haplotype_not_the_reference', [INS, REF], [_unplaced(INS[90:150]), 'N' * 60, REF[10:70]],
      force_alignment=1)
  one('force_alignment_only_the_reference', [REF], [_unplaced(REF[90:150]), 'N' * 60, REF[10:70]], force_alignment=1)
  one('every_haplotype_is_the_reference', [REF, REF.lower(), REF], [REF[10:70], _unplaced(REF[100:160])])
  one('no_unplaced_read', [REF, INS], [REF[10:70], INS[90:150], REF[150:210]])
  one('lower_case_and_n_in_reference_and_reads', [REF, INS], [INS[90:150].lower(), _flip(REF[10:70], 5).replace('A', 'N', 1)],
      )
  return out


def _seeded_window(rng, name, n_reads=None, max_haps=8):
  ref = _bases(rng, rng.randint(150, 400))
  if rng.random() < 0.6:
    p = rng.randint(20, len(ref) - 60)
    unit = _bases(rng, rng.randint(1, 4))
    ref = (ref[:p] + unit * rng.randint(3, 10) + ref[p:])[:400]
  haps = []
  for h in range(rng.randint(1, max_haps)):
    s = ref if not haps or rng.random() < 0.7 else rng.choice(haps)
    for _ in range(rng.randint(0, 3)):
      p = rng.randint(5, len(s) - 20)
      kind = rng.randint(0, 4)
      if kind == 0:
        s = s[:p] + rng.choice('ACGT') + s[p + 1:]
      elif kind == 1:
        s = s[:p] + _bases(rng, rng.randint(1, 10)) + s[p:]
      elif kind == 2:
        s = s[:p] + s[p + rng.randint(1, 10):]
      elif kind == 3:
        s = _bases(rng, rng.randint(1, 10)) + s[rng.randint(1, 10):]
      else:
        s = s[:-rng.randint(1, 10)] + _bases(rng, rng.randint(1, 10))
    haps.append(s)
  if rng.random() < 0.5:
    haps[rng.randrange(len(haps))] = ref
  if rng.random() < 0.3:
    p = rng.randrange(len(ref))
    ref = ref[:p] + 'N' + ref[p + 1:]
  reads = []
  length = rng.randint(40, 120)
  for _ in range(n_reads if n_reads is not None else rng.randint(1, 12)):
    h = rng.choice(haps)
    n = min(length if rng.random() < 0.7 else rng.randint(30, 250), len(h))
    p = rng.randint(0, len(h) - n)
    s = h[p:p + n]
    if rng.random() < 0.4:
      for _ in range(rng.randint(1, 4)):
        q = rng.randint(1, len(s) - 2)
        kind = rng.randint(0, 3)
        s = (s[:q] + rng.choice('ACGT') + s[q + 1:] if kind == 0 else s[:q] + _bases(rng, rng.randint(1, 6)) + s[q:]
             if kind == 1 else s[:q] + s[q + rng.randint(1, 6):] if kind == 2 else s[:q] + 'N' + s[q + 1:])
    if rng.random() < 0.15:
      s = _bases(rng, rng.randint(1, 15)) + s if rng.random() < 0.5 else s + _bases(rng, rng.randint(1, 15))
    s = (s + _bases(rng, 30))[:max(30, min(len(s), 250))]
    reads.append(s)
  return dict(name=name, haplotypes=haps, reads=reads, reference=ref, ref_start=rng.randint(0, 10 ** 9),
              ref_prefix_len=rng.randint(0, 30), ref_suffix_len=rng.randint(0, 30))


def seeded(seed, n_windows, **kw):
  rng = random.Random(seed)
  windows = [_seeded_window(rng, 'seed%d_w%d' % (seed, i), **kw) for i in range(n_windows)]
  options = dict(kmer_size=rng.choice([12, 16, 32]), read_size=len(windows[0]['reads'][0]),
                 normalize_reads=seed % 2, force_alignment=1 if seed % 3 == 0 else 0)
  return case('seeded_%d_%dw' % (seed, n_windows), windows, **options)


def seeded_cases():
  return [seeded(s, 6) for s in range(1, 25)] + [seeded(100 + s, 3, max_haps=40) for s in range(6)]


def read_counts():
  """Windows of 1, 63, 64, 65 and 257 reads."""
  return [case('window_of_%d_reads' % n, _seeded_window(random.Random(500 + n), 'reads%d' % n, n_reads=n, max_haps=3),
               read_size=60) for n in (1, 63, 64, 65, 257)]


def total_reads(total):
  """One call whose reads number `total`: windows of at most 200 reads, so the scan's carry is crossed inside a call."""
  rng = random.Random(7000 + total)
  windows, left = [], total
  while left > 0:
    n = min(left, rng.randint(120, 200))
    windows.append(_seeded_window(rng, 'total%d_w%d' % (total, len(windows)), n_reads=n, max_haps=2))
    left -= n
  return case('call_of_%d_reads' % total, windows, read_size=60)


def tiny_windows(n=300):
  rng = random.Random(4)
  windows = []
  for i in range(n):
    ref = _bases(rng, 150)
    hap = ref[:70] + _bases(rng, rng.randint(1, 4)) + ref[70 + rng.randint(0, 3):]
    windows.append(dict(name='tiny%d' % i, haplotypes=[ref, hap], reads=[hap[40:100], _unplaced(ref[60:120])][:1 + i % 2],
                        reference=ref, ref_start=1000 * i))
  return case('%d_tiny_windows' % n, windows)


def past_the_limits():
  """-> (case, pairs): a window whose haplotype -> reference alignment needs a band past
  DV_LOCAL_ALIGN_DEVICE_MAX_BAND (a 40-base deletion), one with more than DV_LOCAL_ALIGN_DEVICE_MAX_RUNS runs (33
  two-base deletions 9 apart), between windows inside the limits.  pairs[w] = (reference, query) of the pair that
  decides, None for the windows inside: dv_local_align_band says on the host what the device will do with it."""
  rng = random.Random(99)
  ref = _bases(rng, 400)
  wide = ref[:180] + ref[220:]
  many = ''.join(ref[i:i + 9] for i in range(0, 363, 11)) + ref[363:]
  inside = lambda name: window(name, [REF, INS], [INS[90:150], _unplaced(REF[20:80])])      # noqa: E731
  windows = [inside('inside_0'),
             window('band_past_the_cap', [ref, wide], [wide[150:210], ref[10:70]], reference=ref),
             inside('inside_1'),
             window('runs_past_the_cap', [ref, many], [many[100:160], ref[10:70]], reference=ref),
             inside('inside_2')]
  return case('past_the_limits', windows), [None, (ref, wide), None, (ref, many), None]


def all_cases():
  return hand_made() + seeded_cases() + read_counts() + [total_reads(n) for n in (1023, 1024, 1025, 2049)] + \
      [tiny_windows(), past_the_limits()[0]]


_HOST = {}


def host_answer(c):
  """align_windows_batch (the host code) for a case, computed once and shared; callers leave it unchanged."""
  if c['name'] not in _HOST:
    from deepvariant_amd import fast_pass_aligner as F
    _HOST[c['name']] = F.align_windows_batch(c['windows'], c['options'])
  return _HOST[c['name']]


def windows_past_the_limits(c):
  """-> the indices of the windows of `c` the device hands back, worked out on the host: the pairs
  FastPassAligner::collect_alignments lists (every haplotype that differs from the reference against it; every read
  the fast pass left unplaced against every target haplotype), each asked of dv_local_align_band."""
  import ctypes as C
  from deepvariant_amd import _lib
  from deepvariant_amd import fast_pass_aligner as F
  o = c['options']
  scoring = [o.get('match') or 4, o.get('mismatch') or 6, o.get('gap_open') or 8, o.get('gap_extend') or 1]
  over = []
  for i, w in enumerate(c['windows']):
    if not w['reads']:
      continue
    fast = F.fast_pass_batch([w], o)[0]
    score = [0 if d else int(s) for s, d in zip(fast['haplotype_score'], fast['haplotype_discarded'])]
    pairs = [(w['reference'], h) for h in w['haplotypes'] if h != w['reference']]
    targets = [h for h, s in zip(w['haplotypes'], score) if s != 0 or o.get('force_alignment')]
    for r, read in enumerate(w['reads']):
      placed = any(score[h] != 0 and fast['read_position'][h][r] >= 0 and fast['read_score'][h][r] > 0
                   for h in range(len(w['haplotypes'])))
      if not placed:
        pairs += [(h, read.upper()) for h in targets]
    for ref, query in pairs:
      if not ref or not query:
        continue
      band, runs = C.c_int32(), C.c_int32()
      _lib.check(_lib.lib().dv_local_align_band(ref.encode(), query.encode(), *scoring, C.byref(band), C.byref(runs)))
      if band.value > _lib.DV_LOCAL_ALIGN_DEVICE_MAX_BAND or runs.value > _lib.DV_LOCAL_ALIGN_DEVICE_MAX_RUNS:
        over.append(i)
        break
  return over
