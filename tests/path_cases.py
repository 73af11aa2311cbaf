"""Windows for the tests of the realigner's haplotypes from the device (tests/test_debruijn_paths_cpu.py,
tests/test_hip_debruijn_paths.py): the hand-made and the seeded windows of tests/assembly_cases.py, and hand-made
windows at the smallest shapes where pruning, the count of walks and their enumeration in lexicographic order can go
wrong (csrc/debruijn_paths.h has the rule).  A case is (name, ref, reads, options) and is named for what it holds;
tests/test_debruijn_paths_cpu.py asserts on the host's answer that it holds it.  Not a test module."""
from deepvariant_amd import _lib
from tests import assembly_cases as AC

read, options, random_bases = AC.read, AC.options, AC.random_bases

SPACING = 16          # between SNP sites: more than any k these windows are built at, so the bubbles are independent
ARM = 14              # a read reaches this far to either side of its site


def _alt(base, step=1):
  return 'ACGT'[('ACGT'.index(base) + step) % 4]


def _sites(n, first=20):
  return [first + SPACING * i for i in range(n)]


def _bubble_reads(ref, sites):
  """Per site two reads with the other base and two with the reference's, ARM bases to either side."""
  reads = []
  for p in sites:
    alt = ref[:p] + _alt(ref[p]) + ref[p + 1:]
    reads += [read(alt[p - ARM:p + ARM + 1])] * 2 + [read(ref[p - ARM:p + ARM + 1])] * 2
  return reads


def bubbles(n, seed, length=None, **changes):
  """(ref, reads, options): n independent SNP bubbles, 2 ** n walks of len(ref) bytes each."""
  ref = random_bases(seed, length or (2 * 20 + SPACING * (n - 1) + 1))
  return ref, _bubble_reads(ref, _sites(n)), options(**changes)


def near_max_num_paths():
  """T = 8 with max_num_paths 7, 8, 9: T == max is kept, T == max + 1 is dropped; T = 256 at the default, exactly;
  512 walks for a workgroup of 256 to stride over; 2 ** 33 walks, which a 32-bit count without saturation wraps."""
  cases = []
  for limit in (7, 8, 9):
    cases.append(('3 bubbles, max_num_paths %d' % limit,) + bubbles(3, 41, max_num_paths=limit))
  cases.append(('8 bubbles at the default',) + bubbles(8, 42))
  cases.append(('9 bubbles, max_num_paths 1024',) + bubbles(9, 43, max_num_paths=1024))
  cases.append(('33 bubbles',) + bubbles(33, 44))
  return cases


def ordering():
  ref = random_bases(45, 120)
  p, q = 40, 40 + SPACING
  cases = []
  # three alleles at one site
  three = []
  for step in (1, 2):
    alt = ref[:p] + _alt(ref[p], step) + ref[p + 1:]
    three += [read(alt[p - ARM:p + ARM + 1])] * 2
  cases.append(('three-allele site', ref, three + [read(ref[p - ARM:p + ARM + 1])] * 2, options()))
  # a deletion over both SNP sites, and an insertion further on: walks of different lengths
  deleted = ref[:p - 4] + ref[q + 5:]
  inserted = ref[:90] + 'GATTACA' + ref[90:]
  indels = _bubble_reads(ref, [p, q]) + [read(deleted[p - 4 - 20:p - 4 + 20])] * 2 + [read(inserted[90 - 20:97 + 20])] * 2
  cases.append(('deletion over two bubbles and an insertion', ref, indels, options()))
  # the reference's byte right after a branch point is N (between G and T) or lower case (after T): the reads put
  # every base there, so the reference's walk sorts where its byte does, not where an A < C < G < T table puts it
  for name, byte in (('N', 'N'), ('lower-case base', ref[p].lower())):
    odd = ref[:p] + byte + ref[p + 1:]
    reads = []
    for base in 'ACGT':
      alt = ref[:p] + base + ref[p + 1:]
      reads += [read(alt[p - ARM:p + ARM + 1])] * 2
    cases.append(('reference with a %s after a branch point' % name, odd, reads, options()))
  # a walk over more than 256 vertices: the 330-base reference of AC.hand_made(), two SNPs
  long_ref = random_bases(14, 330)
  cases.append(('walks longer than 256 vertices', long_ref, _bubble_reads(long_ref, [100, 200]), options()))
  return cases


def pruning():
  ref = random_bases(46, 120)
  p = 50
  alt = ref[:p] + _alt(ref[p]) + ref[p + 1:]
  other = ref[:80] + _alt(ref[80]) + ref[81:]
  kept = [read(other[80 - ARM:80 + ARM + 1])] * 2           # one real bubble, so that there is something to order
  cases = []
  # the alternative branch is walked twice over its first edges and once over the rest: min_edge_weight cuts it in
  # the middle and its alive start is a dead end
  cases.append(('branch cut by min_edge_weight leaves a dead end', ref,
                kept + [read(alt[p - ARM:p + ARM + 1]), read(alt[p - ARM:p + 4])], options()))
  # alive, but it never comes back to the reference
  astray = ref[30:p] + random_bases(47, 30)
  cases.append(('alive branch that never rejoins', ref, kept + [read(astray)] * 2, options()))
  # starts outside the reference and joins it: alive, but not reachable from the source
  joining = random_bases(48, 30) + ref[40:70]
  cases.append(('read-only start that joins the reference', ref, kept + [read(joining)] * 2, options()))
  # the sink has alive out-edges and the source alive in-edges
  beyond = random_bases(49, 15) + alt + random_bases(50, 15)
  cases.append(('reads past both ends of the reference', ref, kept + [read(beyond)] * 2, options()))
  return cases


def hap_bytes_window(name, length):
  """10 bubbles and max_num_paths 1024: 1024 walks of `length` bytes."""
  return (name,) + bubbles(10, 51, length=length, max_num_paths=1024)


_PER_WALK = _lib.DV_DEBRUIJN_DEVICE_MAX_HAP_BYTES // 1024


def to_the_host():
  """Calls and windows the device leaves to the host: a whole call without pruning or with max_num_paths above
  DV_DEBRUIJN_DEVICE_MAX_PATHS; between small neighbours a window whose haplotypes' text comes just under
  DV_DEBRUIJN_DEVICE_MAX_HAP_BYTES (the device's own), one just over, and AC.limit_windows()'s vertices_over, whose
  graph the graph kernel already hands back."""
  hand = AC.hand_made()
  noisy = next(c for c in hand if c[0] == 'disable_graph_pruning')
  cases = [('disable_graph_pruning=True',) + noisy[1:],
           ('3 bubbles without pruning',) + bubbles(3, 41, disable_graph_pruning=True),
           ('3 bubbles, max_num_paths 2048',) + bubbles(3, 41, max_num_paths=2048)]
  wide = dict(max_num_paths=1024)
  small = [(c[0] + ' (neighbour)', c[1], c[2], options(**wide)) for c in hand[:4]]
  cases += small[:2]
  cases.append(hap_bytes_window('haplotype bytes just under the limit', _PER_WALK - 1))
  cases.append(small[2])
  cases.append(hap_bytes_window('haplotype bytes just over the limit', _PER_WALK + 1))
  cases.append(small[3])
  over = next(c for c in AC.limit_windows() if c[0] == 'vertices_over')
  cases += [(c[0] + ' (neighbour of vertices_over)', c[1], c[2], over[3]) for c in hand[:2]]
  cases.append(over)
  return cases


def general():
  ref = random_bases(11, 90)
  return [('no reads at all', ref, [], options()),
          ('no graph', 'A' * 40, [read('A' * 30), read('A' * 12 + 'C' + 'A' * 12)], options())]


KINDS = {'near_max_num_paths': near_max_num_paths, 'ordering': ordering, 'pruning': pruning, 'to_the_host': to_the_host,
         'general': general}


def hand_made():
  """[(name, ref, reads, options)]: every kind above."""
  return [case for make in KINDS.values() for case in make()]


def all_cases():
  """AC.hand_made(), AC.generated(seed) for AC.SEEDS, and hand_made()."""
  return AC.hand_made() + [c for seed in AC.SEEDS for c in AC.generated(seed)] + hand_made()


def call_key(o):
  """All eight option fields: pruning and the paths depend on every one, so only windows that agree share a call."""
  return (o.min_k, o.max_k, o.step_k, o.min_mapq, o.min_base_quality, o.min_edge_weight, o.max_num_paths,
          bool(o.disable_graph_pruning))


def batches(cases):
  """cases grouped by call_key, in first-seen order: [(options, [case])]."""
  groups = {}
  for case in cases:
    groups.setdefault(call_key(case[3]), (case[3], []))[1].append(case)
  return list(groups.values())
