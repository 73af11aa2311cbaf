"""Regions for the batch phasing entry points (dv_phase_reads_batch / _device): the reference's vectors of
test_direct_phasing_cpu.py as arrays, two seeded generators (small regions; dense ones up to the device limits) and
named cases.  A case is
  {'name', 'n_reads', 'sites': [(start, end, [(bases, is_ref, [(read, is_low_quality), ...]), ...]), ...]}
with the entries of a site in the order DirectPhasing.phase builds them (the is_ref entry first).  The checker is
dv_phase_reads on the region alone (`reference`)."""
import numpy as np

from deepvariant_amd import _lib
from deepvariant_amd import direct_phasing as dp

MAX_READS = _lib.DV_PHASING_DEVICE_MAX_READS
MAX_VERTICES = _lib.DV_PHASING_DEVICE_MAX_VERTICES


def region_arrays(case):
  """-> (candidates, alleles, bases, support_reads, support_low_quality, n_reads), offsets relative to the region."""
  cands = np.zeros(len(case['sites']), dp.CANDIDATE_DTYPE)
  alleles, bases, support, low = [], b'', [], []
  for i, (start, end, entries) in enumerate(case['sites']):
    cands[i] = (start, end, len(alleles), len(entries))
    for text, is_ref, infos in entries:
      raw = b'' if is_ref else text.encode()
      alleles.append((len(bases), len(raw), 1 if is_ref else 0, len(support), len(infos), 0))
      bases += raw
      support += [r for r, _ in infos]
      low += [1 if q else 0 for _, q in infos]
  return (cands, np.array(alleles, dp.ALLELE_DTYPE) if alleles else np.zeros(0, dp.ALLELE_DTYPE), bases,
          np.array(support, np.int32), np.array(low, np.uint8), case['n_reads'])


def reference(case, min_alleles_to_phase):
  """dv_phase_reads on the region alone -> (read_phases, allele_phases, allele_flags)."""
  cands, alleles, bases, support, low, n_reads = region_arrays(case)
  phases = np.zeros(max(n_reads, 1), np.int32)
  allele_phases = np.zeros(max(len(alleles), 1), np.int32)
  allele_flags = np.zeros(max(len(alleles), 1), np.uint8)
  _lib.check(_lib.lib().dv_phase_reads(
      cands.ctypes.data, len(cands), alleles.ctypes.data, len(alleles), bases, len(bases), support.ctypes.data,
      low.ctypes.data, len(support), n_reads, min_alleles_to_phase, phases.ctypes.data, allele_phases.ctypes.data,
      allele_flags.ctypes.data, None, 0))
  return phases[:n_reads], allele_phases[:len(alleles)], allele_flags[:len(alleles)]


def same(got, want):
  return all(np.array_equal(g, w) for g, w in zip(got, want)) and len(got) == len(want)


# ---- the reference's vectors (deepvariant/direct_phasing_test.cc through test_direct_phasing_cpu.py)

def site(start, end, allele_support, ref_support=(), low_quality=()):
  """Reads by their 1-based number as in the vectors; 0 = a read that is not among the region's."""
  def infos(ids):
    return [(i - 1, i in low_quality) for i in ids]
  entries = [('', True, infos(ref_support))] if ref_support else []
  return (start, end, entries + [(allele, False, infos(ids)) for allele, ids in allele_support.items()])


def vector_cases():
  v = []

  def add(name, n_reads, *sites):
    v.append({'name': name, 'n_reads': n_reads, 'sites': list(sites)})
  add('build_graph_simple', 6, site(100, 101, {'A': [1, 2, 3], 'C': [4, 5, 6]}),
      site(105, 106, {'C': [1, 2, 3]}, [4, 5, 6]), site(110, 111, {'T': [1, 2, 3], 'G': [4, 5]}))
  add('low_quality_and_unknown', 5, site(100, 101, {'A': [1, 2, 3], 'C': [4, 5, 0]}, low_quality={3}),
      site(110, 111, {'T': [1, 2, 3], 'G': [4, 5]}, low_quality={3}))
  add('simple', 5, site(100, 101, {'A': [1, 2, 3], 'C': [4, 5]}), site(105, 106, {'C': [1, 2, 4, 5]}),
      site(110, 111, {'T': [1, 2, 3], 'G': [4, 5]}))
  add('error_correction', 5, site(100, 101, {'A': [1, 2, 3], 'C': [4, 5]}), site(105, 106, {'C': [1, 2, 3, 4, 5]}),
      site(110, 111, {'T': [1, 2], 'G': [3, 4, 5]}), site(120, 121, {'T': [1, 2, 3], 'G': [4, 5]}))
  add('changed_order_of_alleles', 5, site(100, 101, {'A': [1, 2, 3], 'C': [4, 5]}),
      site(105, 106, {'C': [1, 2, 3, 4, 5]}), site(110, 111, {'T': [4, 5], 'G': [1, 2, 3]}),
      site(120, 121, {'G': [4, 5], 'T': [1, 2, 3]}))
  add('unphased_read', 5, site(100, 101, {'A': [1, 2, 3], 'C': [4, 5]}), site(105, 106, {'C': [1, 2, 3, 4, 5]}),
      site(110, 111, {'T': [1, 2], 'G': [4, 5, 3]}))
  add('broken_path', 7, site(100, 101, {'A': [1, 2, 3], 'C': [4, 5]}), site(105, 106, {'C': [4, 5], 'G': [6, 7]}),
      site(110, 111, {'T': [6, 7], 'G': [4, 5]}))
  add('broken_path_no_connection', 9, site(100, 101, {'A': [1, 2, 3], 'C': [4, 5]}),
      site(105, 106, {'C': [1, 2, 3], 'G': [4, 5]}), site(110, 111, {'C': [6, 7], 'G': [8, 9]}),
      site(120, 121, {'T': [6, 7], 'G': [8, 9]}))
  add('fully_connected', 6, site(100, 101, {'A': [1, 2, 3], 'C': [4, 5, 6]}),
      site(105, 106, {'C': [4, 5, 1], 'G': [2, 3, 6]}), site(110, 111, {'T': [1, 2, 3], 'G': [4, 5, 6]}))
  add('two_blocks_with_score_tie', 12, site(100, 101, {'A': [1, 2], 'C': [3, 4]}),
      site(110, 111, {'G': [1, 2], 'T': [3, 4]}), site(120, 121, {'A': [5, 6, 7, 8], 'C': [9, 10, 11, 12]}))
  add('one_allele_one_ref_read', 7, site(100, 101, {'C': [4, 5, 6]}, [7]),
      site(110, 111, {'T': [1, 2, 3], 'G': [4, 5, 6]}))
  add('indel_allele', 7, site(100, 102, {'CC': [4, 5, 6], 'A': [1, 2]}, [7]),
      site(110, 111, {'T': [1, 2, 3], 'G': [4, 5, 6]}))
  add('inside_an_indel', 7, site(100, 105, {'A': [1, 2], 'CCCCC': [4, 5]}),
      site(103, 104, {'T': [1, 2, 3], 'G': [4, 5, 6]}), site(110, 111, {'T': [1, 2, 3], 'G': [4, 5, 6]}))
  add('three_ref_reads', 7, site(100, 101, {'C': [4, 5, 6]}, [1, 2, 3]),
      site(110, 111, {'T': [1, 2, 3], 'G': [4, 5, 6]}))
  add('reuse_second', 5, site(120, 121, {'G': [1, 2, 3], 'A': [4, 5]}), site(130, 131, {'T': [1, 2, 3, 4, 5]}))
  add('broken_phase', 13, site(100, 101, {'A': [1, 2, 3, 10], 'C': [4, 5]}),
      site(105, 106, {'C': [1, 2, 3, 10, 11], 'G': [4, 5, 12, 13]}), site(110, 111, {'C': [10, 13], 'G': [11, 12]}),
      site(120, 121, {'T': [6, 7], 'G': [8, 9]}), site(125, 126, {'A': [6, 7], 'T': [8, 9]}))
  add('broken_phase_no_connection', 12, site(100, 101, {'A': [1, 2, 3], 'C': [4, 5, 6]}),
      site(105, 106, {'C': [4, 5, 1], 'G': [2, 3, 6]}), site(110, 111, {'C': [7, 8, 9], 'G': [10, 11, 12]}),
      site(120, 121, {'T': [10, 11, 9], 'G': [7, 8, 12]}))
  add('min_alleles', 5, site(100, 101, {'A': [1, 2, 3], 'C': [4, 5]}), site(110, 111, {'T': [1, 2], 'G': [4, 5]}))
  add('no_reads', 0, site(100, 101, {'A': [0, 0, 0], 'C': [0, 0]}), site(110, 111, {'T': [0, 0], 'G': [0, 0]}))
  return v


EMPTY = {'name': 'empty', 'n_reads': 0, 'sites': []}
NO_CANDIDATES = {'name': 'no_candidates', 'n_reads': 3, 'sites': []}


# ---- seeded generator

def generated_case(seed, n_reads=None, n_sites=None):
  """Two haplotypes over 2-12 substitution sites (SNPs, two-base substitutions, sites with REF as an allele -- with G
  and T beside it so that "REF" sorts between them --, three-allelic sites) plus sites with an indel allele whose span
  may shadow the followers; 4-40 reads, each over a random run of sites, with an error rate, low-quality entries and
  entries of reads that are not the region's; REF support cut to 2 or 3 entries at some sites."""
  rng = np.random.RandomState(seed)
  n_sites = n_sites or int(rng.randint(2, 13))
  n_reads = n_reads or int(rng.randint(4, 41))
  error_rate = (0.0, 0.05, 0.2)[seed % 3]
  plan = []      # (start, end, names, the two haplotypes' alleles)
  pos = 100
  for _ in range(n_sites):
    kind = rng.choice(['snp', 'snp', 'ref', 'gt_ref', 'multi', 'mnp', 'indel'])
    span = 1
    if kind == 'snp':
      names = list(rng.choice(list('ACGT'), 2, replace=False))
    elif kind == 'ref':
      names = ['REF', str(rng.choice(list('ACGT')))]
    elif kind == 'gt_ref':
      names = ['REF', 'G', 'T']
    elif kind == 'multi':
      names = list(rng.choice(list('ACGT'), 3, replace=False))
    elif kind == 'mnp':
      span = 2
      names = [''.join(p) for p in rng.choice(list('ACGT'), (3, 2))]
      names = list(dict.fromkeys(names))
      if len(names) < 2:
        names = ['AC', 'GT']
    else:
      span = int(rng.randint(2, 5))
      names = ['A' * span, 'C']              # the second is a deletion: the site is refused and shadows its span
    names = [str(n) for n in names]
    haps = [int(h) for h in rng.permutation(len(names))[:2]]
    plan.append((pos, pos + span, names, haps))
    pos += int(rng.randint(1, 6)) if kind == 'indel' else span + int(rng.randint(0, 5))
  support = [dict() for _ in plan]          # allele -> [(read, low quality)], in order of first support
  for read in range(n_reads):
    hap = int(rng.randint(2))
    a = int(rng.randint(n_sites))
    b = int(rng.randint(a, n_sites))
    for s in range(a, b + 1):
      names, haps = plan[s][2], plan[s][3]
      allele = haps[hap]
      if rng.rand() < error_rate:
        allele = int(rng.randint(len(names)))
      support[s].setdefault(names[allele], []).append((read, bool(rng.rand() < 0.05)))
  sites = []
  for (start, end, names, _), by_allele in zip(plan, support):
    for infos in by_allele.values():
      if rng.rand() < 0.1:
        infos.insert(int(rng.randint(len(infos) + 1)), (-1, False))
    entries = []
    if by_allele.get('REF'):
      infos = by_allele['REF']
      if rng.rand() < 0.4:
        infos = infos[:int(rng.choice([2, 3]))]
      entries.append(('', True, infos))
    entries += [(name, False, infos) for name, infos in by_allele.items() if name != 'REF']
    sites.append((start, end, entries))
  return {'name': 'generated_%d' % seed, 'n_reads': n_reads, 'sites': sites}


def generated_cases(n):
  return [generated_case(seed) for seed in range(n)]


# ---- dense seeded generator: read sets of 1-16 bitmap words, sites of up to MAX_VERTICES vertices

DENSE_READ_COUNTS = (41, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 320, 511, 512, 513, 767, 1000, 1023,
                     MAX_READS)      # both sides of the 64-read word edges, up to the limit
_TWO_BASE_TEXTS = [a + b for a in 'ACGT' for b in 'ACGT']


def dense_case(seed):
  """2, 3, 4 or 6 haplotypes (the checker does not care about ploidy) over 3-40 sites, each haplotype with one allele
  per site, so that many vertices carry real read sets and real edges.  n_reads is DENSE_READ_COUNTS[seed % 21]; the
  error rate cycles through 0, 0.03 and 0.15, shifted every 21 seeds so that every read count meets each.  Sites: REF
  with A, C, G and T (5 vertices, "REF" between G and T); REF with 7 two-base texts (MAX_VERTICES); 2-8 two-base texts;
  2-4 SNP alleles; REF with one allele; generated_case's indel site, whose span shadows its followers.  A read covers
  a random run of sites, skips a site inside it with probability 0.05 and carries exactly one allele per site (a read
  under two alleles of one site would send the region to the host code); half of the regions have a cut that no read
  crosses, which forces a new block.  5 % of the entries are low quality, a -1 entry goes into 10 % of the lists, REF
  support is cut to 2 or 3 entries at 20 % of the REF sites, and sites left without entries are dropped."""
  rng = np.random.RandomState(1000003 + seed)
  n_reads = DENSE_READ_COUNTS[seed % len(DENSE_READ_COUNTS)]
  error_rate = (0.0, 0.03, 0.15)[(seed + seed // len(DENSE_READ_COUNTS)) % 3]
  n_sites = int(rng.randint(3, 41))
  n_haps = int(rng.choice([2, 3, 4, 6]))
  plan = []      # (start, end, names, the haplotypes' alleles)
  pos = 100
  for _ in range(n_sites):
    kind = str(rng.choice(['ref5', 'ref8', 'texts', 'texts', 'snp', 'ref1', 'indel']))
    span = 1
    if kind == 'ref5':
      names = ['REF', 'A', 'C', 'G', 'T']
    elif kind == 'ref8':
      span = 2
      names = ['REF'] + [_TWO_BASE_TEXTS[int(t)] for t in rng.choice(16, MAX_VERTICES - 1, replace=False)]
    elif kind == 'texts':
      span = 2
      names = [_TWO_BASE_TEXTS[int(t)] for t in rng.choice(16, int(rng.randint(2, MAX_VERTICES + 1)), replace=False)]
    elif kind == 'snp':
      names = [str(t) for t in rng.choice(list('ACGT'), int(rng.randint(2, 5)), replace=False)]
    elif kind == 'ref1':
      names = ['REF', str(rng.choice(list('ACGT')))]
    else:
      span = int(rng.randint(2, 5))
      names = ['A' * span, 'C']              # the second is a deletion: the site is refused and shadows its span
    haps = [int(h) for h in rng.randint(len(names), size=n_haps)]
    plan.append((pos, pos + span, names, haps))
    pos += int(rng.randint(1, 6)) if kind == 'indel' else span + int(rng.randint(0, 5))
  cut = int(rng.randint(1, n_sites)) if rng.rand() < 0.5 else None     # no read has sites on both sides of it
  support = [dict() for _ in plan]          # allele -> [(read, low quality)], in order of first support
  for read in range(n_reads):
    hap = int(rng.randint(n_haps))
    a = int(rng.randint(n_sites))
    b = int(rng.randint(a, n_sites))
    if cut is not None and a < cut <= b:
      if rng.rand() < 0.5:
        b = cut - 1
      else:
        a = cut
    for s in range(a, b + 1):
      if a < s < b and rng.rand() < 0.05:
        continue
      names, haps = plan[s][2], plan[s][3]
      allele = haps[hap]
      if rng.rand() < error_rate:
        allele = int(rng.randint(len(names)))
      support[s].setdefault(names[allele], []).append((read, bool(rng.rand() < 0.05)))
  sites = []
  for (start, end, names, _), by_allele in zip(plan, support):
    if not by_allele:
      continue
    for infos in by_allele.values():
      if rng.rand() < 0.1:
        infos.insert(int(rng.randint(len(infos) + 1)), (-1, False))
    entries = []
    if 'REF' in by_allele:
      infos = by_allele['REF']
      if rng.rand() < 0.2:
        infos = infos[:int(rng.choice([2, 3]))]
      entries.append(('', True, infos))
    entries += [(name, False, infos) for name, infos in by_allele.items() if name != 'REF']
    sites.append((start, end, entries))
  return {'name': 'dense_%d' % seed, 'n_reads': n_reads, 'sites': sites}


def dense_cases(n):
  return [dense_case(seed) for seed in range(n)]


# ---- named cases

def two_haplotypes(name, n_reads, n_sites, pairs=None):
  """Every read carries its haplotype's allele at every site: reads 0, 2, 4 ... one haplotype, the odd ones the other."""
  pairs = pairs or [('A', 'C'), ('G', 'T'), ('C', 'A'), ('T', 'G')]
  sites = []
  for s in range(n_sites):
    x, y = pairs[s % len(pairs)]
    sites.append((100 + 10 * s, 101 + 10 * s, [(x, False, [(r, False) for r in range(0, n_reads, 2)]),
                                                (y, False, [(r, False) for r in range(1, n_reads, 2)])]))
  return {'name': name, 'n_reads': n_reads, 'sites': sites}


def named_cases():
  """Inside the device limits."""
  def infos(*reads):
    return [(r, False) for r in reads]
  cases = [
      # one read per side links 100 to 110: no score advances there and all scores lie within one, so 110 starts a
      # new block in the middle of the region although it has incoming edges
      {'name': 'restart_in_the_middle', 'n_reads': 10, 'sites': [
          (100, 101, [('A', False, infos(0, 1)), ('C', False, infos(2, 3))]),
          (110, 111, [('G', False, infos(0, 4, 5)), ('T', False, infos(2, 6, 7))]),
          (120, 121, [('A', False, infos(4, 5, 8)), ('C', False, infos(6, 7, 9))]),
          (130, 131, [('G', False, infos(4, 5, 8)), ('T', False, infos(6, 7, 9))])]},
      # T at 110 has no read from 100: it is joined to every vertex of 100
      {'name': 'vertex_no_read_reaches', 'n_reads': 9, 'sites': [
          (100, 101, [('A', False, infos(0, 1, 2)), ('C', False, infos(3, 4, 5))]),
          (110, 111, [('G', False, infos(0, 1, 2)), ('T', False, infos(6, 7, 8))]),
          (120, 121, [('A', False, infos(0, 1, 2)), ('C', False, infos(6, 7, 8))])]},
      # the same reads under both alleles' neighbours: every pair at 110 scores the same
      {'name': 'all_pair_scores_equal', 'n_reads': 8, 'sites': [
          (100, 101, [('A', False, infos(0, 1, 2, 3)), ('C', False, infos(4, 5, 6, 7))]),
          (110, 111, [('G', False, infos(0, 1, 4, 5)), ('T', False, infos(2, 3, 6, 7))]),
          (120, 121, [('A', False, infos(0, 1, 4, 5)), ('C', False, infos(2, 3, 6, 7))])]},
      # REF between G and T in text order, with 2 and with 3 reference reads
      {'name': 'ref_between_g_and_t', 'n_reads': 12, 'sites': [
          (100, 101, [('', True, infos(0, 1, 2)), ('T', False, infos(3, 4, 5)), ('G', False, infos(6, 7, 8))]),
          (110, 111, [('', True, infos(0, 1)), ('G', False, infos(3, 4, 5, 2)), ('T', False, infos(6, 7, 8))]),
          (120, 121, [('', True, infos(3, 4, 5)), ('G', False, infos(0, 1, 2)), ('T', False, infos(6, 7, 8, 9))])]},
      two_haplotypes('reads_65', 65, 4),
      two_haplotypes('reads_100', 100, 5),
      two_haplotypes('reads_130', 130, 3),
  ]
  noisy = generated_case(7, n_reads=129, n_sites=9)
  noisy['name'] = 'reads_129_noisy'
  return cases + [noisy]


def edge_cases():
  """Inside the device limits, at the edges of the kernel's arithmetic: scores past 2^16, vertices whose read set is
  empty, sites of one vertex.  (Apart from named_cases, whose length other tests slice.)"""
  def infos(*reads, low=False):
    return [(r, low) for r in reads]
  return [
      # 70 sites of 1024 continuing reads: the score passes 2^16 at the 64th, and both halves of the reads are phased
      two_haplotypes('deep_and_long', MAX_READS, 70),
      # every entry of G at 110 is low quality: its read set is empty, no read reaches it and it is joined to A and C
      {'name': 'vertex_all_low_quality_middle', 'n_reads': 6, 'sites': [
          (100, 101, [('A', False, infos(0, 1, 2)), ('C', False, infos(3, 4, 5))]),
          (110, 111, [('G', False, infos(0, 1, 2, low=True)), ('T', False, infos(3, 4, 5))]),
          (120, 121, [('A', False, infos(0, 1, 2)), ('C', False, infos(3, 4, 5))])]},
      # the same at the block's start: starting scores with n1 = 0
      {'name': 'vertex_all_low_quality_first', 'n_reads': 6, 'sites': [
          (100, 101, [('A', False, infos(0, 1, 2, low=True)), ('C', False, infos(3, 4, 5))]),
          (110, 111, [('G', False, infos(0, 1, 2)), ('T', False, infos(3, 4, 5))]),
          (120, 121, [('A', False, infos(0, 1, 2)), ('C', False, infos(3, 4, 5))])]},
      # three entries make REF a vertex, but none of them is a read of the region
      {'name': 'ref_vertex_of_unknown_reads', 'n_reads': 6, 'sites': [
          (100, 101, [('', True, infos(-1, -1, -1)), ('A', False, infos(0, 1, 2)), ('C', False, infos(3, 4, 5))]),
          (110, 111, [('', True, infos(-1, -1, -1)), ('G', False, infos(0, 1, 2)), ('T', False, infos(3, 4, 5))])]},
      # one vertex, one ordered pair
      {'name': 'single_vertex_sites', 'n_reads': 8, 'sites': [
          (100, 101, [('', True, infos(0, 1, 2, 3))]),
          (110, 111, [('G', False, infos(0, 1, 4, 5)), ('T', False, infos(2, 3, 6, 7))]),
          (120, 121, [('', True, infos(0, 1, 2, 3))])]},
  ]


def at_limit_cases():
  """The largest the device takes: a region at the reads-per-region limit and one at the vertices-per-site limit."""
  pairs = [(a + b) for a in 'ACGT' for b in 'ACGT']
  many = []
  for s in range(3):
    entries = [('', True, [(r, False) for r in range(0, 4)])]
    for k in range(MAX_VERTICES - 1):
      entries.append((pairs[(k + 3 * s) % 16], False, [(r, False) for r in range(4 + 3 * k + s, 4 + 3 * k + s + 3)]))
    many.append((100 + 10 * s, 102 + 10 * s, entries))
  return [two_haplotypes('reads_at_limit', MAX_READS, 3),
          {'name': 'vertices_at_limit', 'n_reads': 4 + 3 * MAX_VERTICES, 'sites': many}]


def over_limit_cases():
  """Legal input that the device hands to the host code: one more read, one more vertex, a read under two alleles of
  one site, the same text twice at one site."""
  pairs = [(a + b) for a in 'ACGT' for b in 'ACGT']
  entries = [('', True, [(0, False), (1, False), (2, False)])]
  entries += [(pairs[k], False, [(3 + 2 * k, False), (4 + 2 * k, False)]) for k in range(MAX_VERTICES)]
  return [
      two_haplotypes('one_read_too_many', MAX_READS + 1, 2),
      {'name': 'one_vertex_too_many', 'n_reads': 3 + 2 * MAX_VERTICES + 1, 'sites': [
          (100, 102, entries), (110, 112, entries)]},
      {'name': 'read_under_two_alleles', 'n_reads': 6, 'sites': [
          (100, 101, [('A', False, [(0, False), (1, False), (2, False)]), ('C', False, [(3, False), (4, False)])]),
          (110, 111, [('G', False, [(0, False), (1, False), (3, False)]),
                      ('T', False, [(3, False), (4, False), (5, False)])]),
          (120, 121, [('A', False, [(0, False), (1, False)]), ('C', False, [(3, False), (4, False), (5, False)])])]},
      {'name': 'same_text_twice', 'n_reads': 6, 'sites': [
          (100, 101, [('A', False, [(0, False), (1, False)]), ('A', False, [(2, False), (3, False)])]),
          (110, 111, [('G', False, [(0, False), (1, False)]), ('T', False, [(2, False), (3, False)])])]},
  ]


UNORDERED = {'name': 'unordered', 'n_reads': 6, 'sites': [
    (105, 106, [('A', False, [(0, False), (1, False)]), ('C', False, [(3, False), (4, False)])]),
    (100, 101, [('A', False, [(0, False), (1, False)]), ('C', False, [(3, False), (4, False)])]),
    (110, 111, [('A', False, [(0, False), (1, False)]), ('C', False, [(3, False), (4, False)])])]}


def run_batch(cases, min_alleles_to_phase, device, stream=0):
  """-> ([(read_phases, allele_phases, allele_flags)] per case, stats)."""
  return dp.phase_arrays([region_arrays(c) for c in cases], min_alleles_to_phase, device=device, stream=stream,
                         with_stats=True)

