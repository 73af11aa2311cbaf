"""dv_gvcf_merge, the host code of the gVCF merge (csrc/gvcf_merge.h), against the sequential
loop of tests/gvcf_merge_cases.py on every named case and on seeded random layouts.  No GPU."""
import numpy as np
import pytest

from deepvariant_amd import postprocess_variants as pp
from tests import gvcf_merge_cases as M

CASES = M.named_cases()


def n_blocks(layout):
  return sum(len(blocks) for blocks, _ in layout)


@pytest.mark.parametrize('name', sorted(CASES))
def test_named_case_equals_the_sequential_loop(name):
  layout = CASES[name]
  got = pp.merge_blocks_and_variants(*M.arguments(layout))
  M.assert_result(got, M.expected(layout), layout)
  M.assert_permutation(got, n_blocks(layout))


def test_known_answers():
  """Worked by hand: block [0, 10) around the variant [3, 5), block [20, 30) under the variant [25, 40)."""
  got = pp.merge_blocks_and_variants([0, 2], [0, 2], [0, 20], [10, 30], [3, 25], [5, 40])
  assert got.piece_start.tolist() == [0, 5, 20] and got.piece_end.tolist() == [3, 10, 25]
  assert got.piece_block.tolist() == [0, 0, 1]
  assert got.piece_slot.tolist() == [0, 2, 3] and got.var_slot.tolist() == [1, 4]
  # a variant that only touches a block comes before it and takes nothing from it
  got = pp.merge_blocks_and_variants([0, 1], [0, 1], [10], [20], [5], [10])
  assert (got.piece_start.tolist(), got.piece_end.tolist(), got.piece_slot.tolist(), got.var_slot.tolist()) == (
      [10], [20], [1], [0])


def test_random_layouts_equal_the_sequential_loop():
  rng = np.random.default_rng(20260422)
  pieces = variants = 0
  for _ in range(20000):
    layout = M.random_layout(rng)
    got = pp.merge_blocks_and_variants(*M.arguments(layout))
    M.assert_result(got, M.expected(layout), layout)
    M.assert_permutation(got, n_blocks(layout))
    pieces += got.piece_slot.size
    variants += got.var_slot.size
  assert pieces > 40000 and variants > 40000          # the layouts are not trivially empty


def test_a_long_contig_equals_the_sequential_loop():
  rng = np.random.default_rng(7)
  layout = [M.big_group(rng, 3000, 500), M.big_group(rng, 0, 40), M.big_group(rng, 2500, 0), M.big_group(rng, 1200, 900)]
  got = pp.merge_blocks_and_variants(*M.arguments(layout))
  M.assert_result(got, M.expected(layout))
  M.assert_permutation(got, n_blocks(layout))


@pytest.mark.parametrize('arguments, message', [
    (([0, 2], [0, 0], [10, 0], [20, 5], [], []), 'out of order or overlaps'),          # blocks unsorted
    (([0, 2], [0, 0], [0, 9], [10, 20], [], []), 'out of order or overlaps'),          # blocks overlap
    (([0, 0], [0, 2], [], [], [5, 4], [6, 9]), 'variant 1 is out of order'),           # starts descend
    (([0, 0], [0, 2], [], [], [5, 5], [9, 6]), 'variant 1 is out of order'),           # same start, ends descend
    (([0, 1], [0, 0], [5], [5], [], []), 'block 0 is empty'),
    (([0, 0], [0, 1], [], [], [7], [6]), 'variant 0 is empty'),
    (([0, 2, 1, 2], [0, 0, 0, 0], [0, 10], [5, 20], [], []), 'descend at group 1'),    # offsets do not ascend
    (([1, 2], [0, 0], [0, 10], [5, 20], [], []), 'must start at 0'),
])
def test_refused_inputs(arguments, message):
  with pytest.raises(Exception, match=message):
    pp.merge_blocks_and_variants(*arguments)


def test_order_is_per_group():
  """The second group's records start below the first group's: legal, the groups are contigs."""
  layout = [([(100, 200)], [(150, 151)]), ([(0, 50)], [(10, 11)])]
  got = pp.merge_blocks_and_variants(*M.arguments(layout))
  M.assert_result(got, M.expected(layout), layout)
  assert got.var_slot.tolist() == [1, 4]


def test_python_checks_its_arguments():
  with pytest.raises(ValueError, match='one end per start'):
    pp.merge_blocks_and_variants([0, 1], [0, 0], [0], [], [], [])
  with pytest.raises(ValueError, match='must end at the number'):
    pp.merge_blocks_and_variants([0, 2], [0, 0], [0], [5], [], [])
  with pytest.raises(ValueError, match='one entry per group'):
    pp.merge_blocks_and_variants([0, 1], [0], [0], [5], [], [])


def test_scan_chunk_is_exported():
  assert pp.merge_scan_chunk() >= 64


def test_layouts_around_the_scan_chunk_equal_the_sequential_loop():
  """The layouts of the device test (tests/test_hip_gvcf_merge.py), which compares with the host code."""
  for name, layout in M.chunk_cases(pp.merge_scan_chunk()).items():
    got = pp.merge_blocks_and_variants(*M.arguments(layout))
    M.assert_result(got, M.expected(layout), name)
    M.assert_permutation(got, n_blocks(layout))
  c = pp.merge_scan_chunk()
  got = pp.merge_blocks_and_variants(*M.arguments(M.chunk_cases(c)['long_variant_across_chunks']))
  # blocks 0..4 whole or cut by their one-base variant, block 5 up to the long variant, nothing until its end
  assert got.piece_block.tolist()[:12] == [0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 2 * c + 50]
