"""Inputs for the native gVCF rows, shared by tests/test_gvcf_rows_cpu.py and
tests/test_hip_gvcf_rows.py: the layouts of tests/gvcf_merge_cases.py filled with block fields and variant records from a
seeded generator, the number edges as one-block calls, and the reference of every comparison -- the Python formatter,
pp.gvcf_rows, joined and encoded.

The FASTA cycles through ACGT and every block's own ref_base is N, so a row shows where its base came from.
"""
import numpy as np

from deepvariant_amd import allelecounter
from deepvariant_amd import postprocess_variants as pp
from tests import gvcf_merge_cases as M

DTYPE = allelecounter.GVCF_BLOCK_DTYPE


class CyclingReference:
  """get_bases alone: base i of every contig is 'ACGT'[i % 4]."""

  def __init__(self):
    self.fetches = []

  def get_bases(self, contig, start, end):
    self.fetches.append((contig, start, end))
    return np.frombuffer(b'ACGT', np.uint8)[np.arange(start, end) % 4].tobytes().decode()


def block(start, end, likelihoods=(-0.0, -3.0, -30.0), gq=30, min_dp=12, med_dp=-1, valid=1, base='N'):
  return (start, end, list(likelihoods), gq, min_dp, med_dp, ord(base), valid, (0, 0))


def record(contig, start, end, rng, alt_length=None):
  """A finished record with one or two alts; its row's content is arbitrary but seeded."""
  n_alts = 1 if alt_length else int(rng.integers(1, 3))
  alts = ['ACGT'[int(rng.integers(0, 4))] * (alt_length or int(rng.integers(1, 4))) for _ in range(n_alts)]
  gls = (-rng.random((n_alts + 1) * (n_alts + 2) // 2) * 20).tolist()
  ad = rng.integers(0, 60, size=n_alts + 1).tolist()
  return pp.VcfRecord(reference_name=contig, start=start, end=end, reference_bases='G' * min(end - start, 12),
                      alternate_bases=alts, quality=float(rng.integers(0, 700)) / 10, filter='PASS',
                      genotype=[0, int(rng.integers(0, n_alts + 1))], gq=int(rng.integers(0, 99)), genotype_likelihood=gls,
                      dp=sum(ad), ad=ad, vaf=[v / max(sum(ad), 1) for v in ad[1:]], call_set_name='s')


def fill(layout, seed=3, med_dp='some'):
  """layout: groups of (blocks, variants) as gvcf_merge_cases makes them -> (records, blocks_by_contig, contigs).
  Group g is the contig c<g>; it is as long as its last block and one base more, so a variant may end past it.
  med_dp: 'some' blocks carry one, 'all' or 'none'."""
  rng = np.random.default_rng(seed)
  records, blocks_by_contig, contigs = [], {}, []
  for g, (spans, variants) in enumerate(layout):
    name = 'c%d' % g
    contigs.append((name, (max(e for _, e in spans) if spans else 1000) + 1))
    rows = []
    for s, e in spans:
      med = -1 if med_dp == 'none' or (med_dp == 'some' and rng.random() < 0.3) else int(rng.integers(0, 200))
      rows.append(block(s, e, (-rng.random(3) * rng.choice([1.0, 30.0])).tolist(), int(rng.integers(0, 100)),
                        int(rng.integers(0, 300)), med, int(rng.integers(0, 2))))
    if rows:
      blocks_by_contig[name] = np.array(rows, DTYPE)
    records.extend(record(name, s, e, rng) for s, e in variants)
  return records, blocks_by_contig, contigs


def reference(records, blocks_by_contig, contigs):
  """The parent's Python formatter over the host merge -> (the body's bytes, its rows as bytes, med_dp)."""
  rows, med_dp = pp.gvcf_rows(records, blocks_by_contig, CyclingReference(), contigs)
  return ''.join(rows).encode(), [row.encode() for row in rows], med_dp


def assert_body(body, want, n_pieces=None):
  """body: a GvcfBody asked for with want_row_off; want: `reference`'s."""
  text, rows, med_dp = want
  assert body.text == text
  assert body.med_dp == med_dp
  off = body.row_off.tolist()
  assert len(off) == len(rows) + 1 and off[0] == 0 and off[-1] == len(text)
  assert [body.text[a:b] for a, b in zip(off[:-1], off[1:])] == rows
  if n_pieces is not None:
    assert body.n_pieces == n_pieces


# ---- the number edges, each a one-block call: {name: (contig name, [blocks])}
def number_edges():
  edges = {}
  for start in (0, 8, 9, 98, 99, 999_999_998, 999_999_999, 2 ** 31, 10 ** 12 - 1):
    edges['start_%d' % start] = ('chr1', [block(start, start + 1)])
    edges['start_%d_longer' % start] = ('chr1', [block(start, start + 2)])
  for value in (0, 9, 10, 99, 100, 2 ** 31 - 1, -7):
    edges['gq_%d' % value] = ('chr1', [block(5, 50, gq=value)])
    edges['min_dp_%d' % value] = ('chr1', [block(5, 50, min_dp=value)])
  edges['med_dp_missing_among_present'] = ('chr1', [block(5, 50, med_dp=17), block(50, 60, med_dp=-1), block(70, 80, med_dp=0)])
  edges['med_dp_all_missing'] = ('chr1', [block(5, 50), block(50, 60)])
  edges['med_dp_large'] = ('chr1', [block(5, 50, med_dp=2 ** 31 - 1)])
  edges['no_valid_gl'] = ('chr1', [block(5, 50, valid=0)])
  edges['valid_gl'] = ('chr1', [block(5, 50, valid=1)])
  edges['name_of_1_byte'] = ('c', [block(5, 50)])
  edges['name_of_40_bytes'] = ('chrUn_' + 'K' * 34, [block(5, 50)])
  # -10 GL exactly on a half, and the two zeros
  halves = {'0.5': -0.05, '1.5': -0.15, '2.5': -0.25, '12.5': -1.25, '-30007.5': 3000.75}
  for text, gl in halves.items():
    assert -10.0 * gl == float(text)
    edges['pl_half_%s' % text] = ('chr1', [block(5, 50, likelihoods=(gl, -4.0, -0.0))])
    edges['pl_half_%s_lowest' % text] = ('chr1', [block(5, 50, likelihoods=(-7.0, gl, -3.3))])
  edges['pl_negative_zero'] = ('chr1', [block(5, 50, likelihoods=(0.0, 0.0, -1.0))])       # -10 * 0.0 is -0.0
  edges['pl_positive_zero'] = ('chr1', [block(5, 50, likelihoods=(-0.0, -0.0, -1.0))])
  edges['pl_near_the_limit'] = ('chr1', [block(5, 50, likelihoods=(-9.0e14, 0.0, 9.0e14))])  # |10 GL| just below 2^53
  return edges


def edge_arguments(edge):
  """-> (records, blocks_by_contig, contigs) of one number edge."""
  name, blocks = edge
  return [], {name: np.array(blocks, DTYPE)}, [(name, 2 * 10 ** 12)]


def variant_cases():
  """{name: (records, blocks_by_contig, contigs)}: what a layout of spans alone does not say."""
  rng = np.random.default_rng(17)
  cases = {}
  # a variant that ends at the contig's length: its end has no base, and no piece starts there
  cases['variant_ends_at_the_contig_length'] = (
      [record('chr1', 95, 100, rng), record('chr1', 20, 23, rng)], {'chr1': np.array([block(10, 60), block(60, 100)], DTYPE)},
      [('chr1', 100)])
  # a row of 5,000 bytes and more
  cases['long_variant_row'] = (
      [record('chr1', 30, 31, rng, alt_length=4950), record('chr1', 40, 42, rng)],
      {'chr1': np.array([block(10, 60, med_dp=3)], DTYPE)}, [('chr0', 10), ('chr1', 100)])
  return cases


def plain_arguments(layout, seed=9, long_row=None):
  """layout -> pp.gvcf_rows_native's arguments as a dict, filled by array: for layouts too large to make a record per
  variant.  Variant j's row is 'v<j>' and 10 to 200 more bytes; long_row: the variant whose row takes 5,000 more."""
  rng = np.random.default_rng(seed)
  block_off, var_off, b_start, b_end, v_start, v_end = M.arguments(layout)
  blocks = np.zeros(b_start.size, DTYPE)
  blocks['start'], blocks['end'] = b_start, b_end
  blocks['likelihoods'] = -rng.random((b_start.size, 3)) * 40
  blocks['gq'] = rng.integers(0, 100, b_start.size)
  blocks['min_dp'] = rng.integers(0, 1000, b_start.size)
  blocks['med_dp'] = rng.integers(-1, 1000, b_start.size)
  blocks['ref_base'] = ord('N')
  blocks['has_valid_gl'] = rng.integers(0, 2, b_start.size)
  lengths = rng.integers(10, 200, v_start.size)
  rows = [b'v%d\t%s\n' % (j, b'x' * (int(n) + (5000 if j == long_row else 0))) for j, n in enumerate(lengths.tolist())]
  var_text_off = np.zeros(len(rows) + 1, np.int64)
  np.cumsum([len(r) for r in rows], out=var_text_off[1:])
  names = [b'c%d' % g for g in range(len(layout))]
  name_off = np.zeros(len(names) + 1, np.int64)
  np.cumsum([len(n) for n in names], out=name_off[1:])
  return dict(block_off=block_off, var_off=var_off, blocks=blocks, var_start=v_start, var_end=v_end,
              var_end_base=np.frombuffer(b'ACGT', np.uint8)[v_end % 4], var_text_off=var_text_off, var_text=b''.join(rows),
              name_off=name_off, names=b''.join(names))


def split_blocks(n_blocks, cut):
  """n_blocks blocks of ten bases without gaps; a one-base variant inside every block of `cut`.  A cut block leaves two
  pieces, so the rows are n_blocks + 2 len(cut), and the variant in block k takes slot k + 1 + 2 (the cuts before k)."""
  return [([(10 * i, 10 * i + 10) for i in range(n_blocks)], [(10 * k + 3, 10 * k + 4) for k in sorted(cut)])]
