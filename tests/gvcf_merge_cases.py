"""Layouts of gVCF reference blocks and variant records for the merge, and the contract as a
plain sequential loop: merge_variants_and_nonvariants as the section states it, two streams and `lessthan`.  It shares
no code with the product and knows nothing of running maxima, bisections or slots.

A layout is a list of groups (contigs); a group is (blocks, variants), lists of (start, end).  Blocks are sorted and
disjoint, variants sorted by (start, end).
"""
import numpy as np


def sequential_merge(blocks, variants):
  """One group.  -> the merged sequence: ('v', j) for variant j, ('b', i, start, end) for a piece of block i."""
  out = []
  bi, vi = 0, 0
  block = (blocks[0][0], blocks[0][1]) if blocks else None

  def next_block():
    nonlocal bi, block
    bi += 1
    block = (blocks[bi][0], blocks[bi][1]) if bi < len(blocks) else None

  def lessthan(a, b):
    return a is not None and (b is None or a[1] <= b[0])

  while block is not None or vi < len(variants):
    variant = variants[vi] if vi < len(variants) else None
    if lessthan(variant, block):
      out.append(('v', vi))
      vi += 1
    elif lessthan(block, variant):
      out.append(('b', bi, block[0], block[1]))
      next_block()
    else:
      if block[0] < variant[0]:
        out.append(('b', bi, block[0], variant[0]))
      if block[1] > variant[1]:
        block = (variant[1], block[1])
      else:
        next_block()
  return out


def expected(layout):
  """The whole call by the sequential loop -> dict of the arrays the native code returns."""
  piece_start, piece_end, piece_block, piece_slot, var_slot = [], [], [], [], []
  slot, block_base = 0, 0
  for blocks, variants in layout:
    slots_of = [None] * len(variants)
    for item in sequential_merge(blocks, variants):
      if item[0] == 'v':
        slots_of[item[1]] = slot
      else:
        piece_block.append(block_base + item[1])
        piece_start.append(item[2])
        piece_end.append(item[3])
        piece_slot.append(slot)
      slot += 1
    var_slot.extend(slots_of)
    block_base += len(blocks)
  return {'piece_start': np.array(piece_start, np.int64), 'piece_end': np.array(piece_end, np.int64),
          'piece_block': np.array(piece_block, np.int32), 'piece_slot': np.array(piece_slot, np.int64),
          'var_slot': np.array(var_slot, np.int64)}


def arguments(layout):
  """-> (block_off, var_off, block_start, block_end, var_start, var_end), what the merge functions take."""
  block_off, var_off = [0], [0]
  b, v = [], []
  for blocks, variants in layout:
    b.extend(blocks)
    v.extend(variants)
    block_off.append(len(b))
    var_off.append(len(v))
  b = np.array(b, np.int64).reshape(-1, 2)
  v = np.array(v, np.int64).reshape(-1, 2)
  return (np.array(block_off, np.int64), np.array(var_off, np.int64), b[:, 0].copy(), b[:, 1].copy(), v[:, 0].copy(),
          v[:, 1].copy())


FIELDS = ('piece_start', 'piece_end', 'piece_block', 'piece_slot', 'var_slot')


def assert_result(got, want, layout=None):
  """got: a MergedBlocks; want: `expected` or another MergedBlocks."""
  for field in FIELDS:
    a = getattr(got, field)
    b = want[field] if isinstance(want, dict) else getattr(want, field)
    assert a.dtype == b.dtype and a.shape == b.shape and (a == b).all(), (field, layout)


def assert_permutation(got, n_blocks):
  slots = np.concatenate([got.piece_slot, got.var_slot])
  assert (np.sort(slots) == np.arange(slots.size)).all()
  assert got.piece_slot.size <= n_blocks + got.var_slot.size            # P <= B + V


def named_cases():
  """{name: layout}: the smallest shapes that can break the rule."""
  three = [(0, 10), (10, 20), (25, 40)]
  return {
      'no_variants': [(three, [])],
      'no_blocks': [([], [(3, 4), (3, 9), (20, 21)])],
      'nothing': [([], [])],
      'no_groups': [],
      'variant_equals_block': [(three, [(10, 20)])],
      'variant_at_block_start': [(three, [(10, 11)])],
      'variant_at_block_end': [(three, [(19, 20)])],
      'variant_inside_block': [(three, [(12, 15)])],
      'variant_touches_block': [(three, [(20, 25)])],                   # end == the next block's start
      'over_several_blocks': [([(0, 10), (10, 20), (20, 30), (30, 40), (40, 50)], [(5, 45)])],
      'nested_variants': [(three, [(2, 18), (4, 6)])],
      'nested_then_beyond': [(three, [(2, 30), (4, 6), (12, 13), (31, 32)])],
      'identical_variants': [(three, [(12, 14), (12, 14)])],
      'in_gap_before_and_after': [([(10, 20), (30, 40)], [(2, 3), (22, 24), (45, 50), (60, 61)])],
      'back_to_back_variants': [(three, [(10, 15), (15, 20), (20, 26)])],
      'same_start_growing_ends': [(three, [(5, 6), (5, 12), (5, 27)])],
      'middle_group_empty': [(three, [(12, 15)]), ([], []), ([(0, 7)], [(3, 4)])],
      'blocks_only_then_variants_only': [(three, []), ([], [(1, 2)]), (three, [(0, 40)])],
      # the running maximum of the variant ends restarts with every group: a group whose first variant is longer than
      # everything before it, and one that follows a group whose last variant is longer than everything in it
      'long_first_variant_in_second_group': [([(0, 10), (10, 20)], [(2, 3)]), ([(0, 10), (10, 20)], [(1, 19), (5, 6)])],
      'long_last_variant_in_first_group': [([(0, 10)], [(2, 1000)]), ([(0, 10), (10, 20), (500, 600)], [(12, 13)])],
  }


def random_group(rng, max_blocks=6, max_variants=6, span=60):
  """Gaps between blocks, nested and identical variants, variants in gaps and past both ends."""
  cuts = np.sort(rng.choice(np.arange(5, span), size=2 * rng.integers(0, max_blocks + 1), replace=False))
  blocks = []
  for k in range(0, len(cuts), 2):
    blocks.append((int(cuts[k]), int(cuts[k + 1])))
    if blocks[-1][0] > 0 and len(blocks) > 1 and rng.random() < 0.4:            # flush against the one before
      blocks[-1] = (blocks[-2][1], blocks[-1][1])
  variants = []
  for _ in range(rng.integers(0, max_variants + 1)):
    if variants and rng.random() < 0.15:
      variants.append(variants[rng.integers(0, len(variants))])                # identical
      continue
    start = int(rng.integers(0, span + 5))
    length = 1 if rng.random() < 0.5 else int(rng.integers(1, 25))
    variants.append((start, start + length))
  return blocks, sorted(variants)


def random_layout(rng):
  return [random_group(rng) for _ in range(rng.integers(1, 4))]


def big_group(rng, n_blocks, n_variants, gap_every=7):
  """A long contig: blocks of 1..40 bases with a gap now and then, short variants with a long one now and then."""
  lengths = rng.integers(1, 41, size=n_blocks)
  gaps = np.where(rng.integers(0, gap_every, size=n_blocks) == 0, rng.integers(1, 30, size=n_blocks), 0)
  ends = np.cumsum(lengths + gaps)
  starts = ends - lengths
  span = int(ends[-1]) + 50 if n_blocks else 1000
  v_start = np.sort(rng.integers(0, span, size=n_variants))
  v_len = np.where(rng.integers(0, 50, size=n_variants) == 0, rng.integers(40, 400, size=n_variants),
                   rng.integers(1, 4, size=n_variants))
  v_end = v_start + v_len
  order = np.lexsort((v_end, v_start))
  return (list(zip(starts.tolist(), ends.tolist())), list(zip(v_start[order].tolist(), v_end[order].tolist())))


def chunk_cases(c, seed=11):
  """{name: layout} around the device scans' chunk of c elements: a carry crosses from one workgroup's chunk to the next
  at multiples of c, in the running maximum of the variant ends and in the sum of the piece counts."""
  rng = np.random.default_rng(seed)
  cases = {}
  for n in (c - 1, c, c + 1, 2 * c + 1):
    cases['both_%d' % n] = [big_group(rng, n, n)]
    cases['blocks_%d_variants_few' % n] = [big_group(rng, n, 3)]
    cases['variants_%d_blocks_few' % n] = [big_group(rng, 3, n)]
  # blocks of ten bases without gaps, a one-base variant in each of the first 2c + 1 -- and variant 5 reaches from the
  # first chunk over every block up to the third chunk: the maximum's carry crosses two chunk edges, and the blocks
  # under it leave nothing
  blocks = [(10 * i, 10 * i + 10) for i in range(3 * c)]
  variants = [(10 * j + 3, 10 * j + 4) for j in range(2 * c + 1)]
  variants[5] = (53, 10 * (2 * c + 50) + 5)
  cases['long_variant_across_chunks'] = [(blocks, sorted(variants))]
  # a group boundary exactly at a chunk edge, of the variants and of the blocks: the first group ends with a variant
  # longer than everything, the second starts over at position 0
  first = ([(10 * i, 10 * i + 10) for i in range(c)], [(10 * j + 3, 10 * j + 4) for j in range(c - 1)] + [(10 * c - 5, 10 ** 9)])
  second = ([(10 * i, 10 * i + 10) for i in range(c + 1)], [(10 * j + 3, 10 * j + 4) for j in range(c + 1)])
  cases['group_boundary_at_chunk_edge'] = [first, second]
  cases['empty_group_at_chunk_edge'] = [first, ([], []), second, ([], [])]
  return cases


def large_layout(seed=5):
  """About 300,000 blocks and 40,000 variants in four groups."""
  rng = np.random.default_rng(seed)
  return [big_group(rng, 90000, 12000), big_group(rng, 60000, 8000), big_group(rng, 110000, 5000),
          big_group(rng, 40000, 15000)]
