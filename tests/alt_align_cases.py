"""Seeded cases for the alt-aligned realignment entry points (dv_alt_align_batch[_device], alt_align_table):
shared by tests/test_alt_align_abi_cpu.py (which asserts, through host code alone, that every kind below really
occurs) and tests/test_hip_alt_align.py.

A batch: dict(name, reads=[Read], starts=[untrimmed starts], items=[(first_row, n_rows, target, ref_start,
read_size)], targets=[str], cfg=aligner options, kinds={kind: (item, row within the item)}).  Targets measure
60-260 bytes, reads 8-230.  Targets are drawn from C / G / T so that a poly-A read aligns nowhere."""
import numpy as np

from deepvariant_amd import dv_types as T

# gap_extend 1: with it the host aligner writes "2D6I" for the pair of kind 'unnormalised' (an insertion run
# beside a deletion run), where gap_extend 2 prefers mismatches
CFG = dict(match=4, mismatch=6, gap_open=8, gap_extend=1, kmer_size=16, max_num_of_mismatches=2,
           realignment_similarity_threshold=0.16934)
REF_START = 1000


class Ref:
  """What realign_reads_to_haplotype asks of a reference reader (K_REF_ALIGN_MARGIN is 0: no bases are fetched)."""

  def n_bases(self, contig):
    return 1 << 30

  def get_bases(self, contig, start, end):
    raise AssertionError('no reference padding is expected')


def _seq(rng, n, alphabet='CGT'):
  return ''.join(alphabet[int(i)] for i in rng.integers(0, len(alphabet), size=n))


def _other(base):
  return {'C': 'G', 'G': 'T', 'T': 'C', 'A': 'C', 'N': 'C'}[base]


def _mutate(seq, positions):
  s = list(seq)
  for p in positions:
    s[p] = _other(s[p])
  return ''.join(s)


def read_size_of(seqs):
  return len(seqs[0]) if seqs and len(seqs[0]) > 15 else 200


def _reads(rng, seqs, tag):
  reads, starts = [], []
  for k, s in enumerate(seqs):
    pos = REF_START + int(rng.integers(0, 50))
    read = T.Read(fragment_name='%s%03d' % (tag, int(rng.integers(0, max(len(seqs) // 2, 1)))),
                  read_number=int(rng.integers(0, 2)), number_reads=2, fragment_length=int(rng.integers(-500, 500)),
                  aligned_sequence=s, aligned_quality=bytes(rng.integers(0, 60, size=len(s)).astype(np.uint8)),
                  alignment=T.LinearAlignment(position=T.Position('chr1', pos, bool(rng.integers(0, 2))),
                                              mapping_quality=int(rng.integers(0, 70)), cigar=[T.CigarUnit(1, len(s))]))
    if k % 3 == 0:
      read.info['HP'] = T.ListValue(values=[T.Value(int_value=int(rng.integers(0, 3)))])
    reads.append(read)
    starts.append(pos - int(rng.integers(0, 400)))      # the untrimmed start: what read_sort_pos carries
  return reads, starts


def _item(first, seqs, target_index, ref_start=REF_START):
  return (first, len(seqs), target_index, ref_start, read_size_of(seqs))


def kinds_batch():
  rng = np.random.default_rng(20261020)
  t = _seq(rng, 200)
  n = len(t)
  short_target = _seq(rng, 60)
  left, right = _seq(rng, 28) + 'CC', 'G' + _seq(rng, 29)
  n_target = left + 'NN' + right
  kinds, seqs = {}, []

  def add(kind, s):
    kinds[kind] = (0, len(seqs))
    seqs.append(s)

  add('fast_p0', t[0:60])
  add('fast_pend', t[n - 50:])
  add('fast_max_mismatches', _mutate(t[40:120], [20, 50]))
  add('one_more_mismatch', _mutate(t[40:120], [18, 40, 62]))
  add('short', t[30:42])
  add('lower_case', t[70:130].lower())
  add('insertion3', t[20:60] + 'AAA' + t[60:100])
  add('deletion5', t[100:130] + t[135:170])
  add('unrelated', 'A' * 40)
  add('insertion40', t[10:70] + 'A' * 40 + t[70:130])
  main = list(seqs)
  longer = [_seq(rng, 30) + short_target + _seq(rng, 40), short_target[5:50]]
  kinds['longer_than_target'] = (1, 0)
  # the inserted CCCC sits in the C run the target's left flank ends with, in front of two N
  odd = [left + 'CCCCNN' + right, left + 'NN' + right]
  kinds['unnormalised'] = (2, 0)
  all_seqs = main + longer + odd
  reads, starts = _reads(rng, all_seqs, 'k')
  items = [_item(0, main, 0), _item(len(main), longer, 1), _item(len(main) + len(longer), odd, 2, REF_START + 500),
           (3, 0, 0, REF_START, 200)]                       # an item with no reads
  kinds['empty_item'] = (3, 0)
  return dict(name='kinds', reads=reads, starts=starts, items=items, targets=[t, short_target, n_target], cfg=dict(CFG),
              kinds=kinds)


def _edited(rng, t):
  """A read drawn from target t: a substring, clean or with mismatches, an insertion, a deletion or overhangs."""
  n = len(t)
  length = int(rng.integers(8, min(200, n) + 1))
  s0 = int(rng.integers(0, n - length + 1))
  s = t[s0:s0 + length]
  kind = int(rng.integers(0, 8))
  if kind == 1:
    s = _mutate(s, sorted(set(rng.integers(0, len(s), size=int(rng.integers(1, 5))).tolist())))
  elif kind == 2 and len(s) > 20:
    at = int(rng.integers(8, len(s) - 8))
    s = s[:at] + 'A' * int(rng.integers(1, 7)) + s[at:]
  elif kind == 3 and len(s) > 30:
    at = int(rng.integers(10, len(s) - 14))
    s = s[:at] + s[at + int(rng.integers(1, 6)):]
  elif kind == 4:
    s = _seq(rng, int(rng.integers(1, 12)), 'ACGT') + s + _seq(rng, int(rng.integers(1, 12)), 'ACGT')
  elif kind == 5 and len(s) > 30:
    at = int(rng.integers(10, len(s) - 14))
    s = s[:at] + _seq(rng, int(rng.integers(1, 5)), 'ACGT') + s[at + int(rng.integers(1, 5)):]
  return s[:230]


def shared_rows_batch():
  """Two items over the same rows with different targets (two alts of one candidate)."""
  rng = np.random.default_rng(20261021)
  t = _seq(rng, 180)
  t2 = t[:90] + t[93:]
  seqs = [_edited(rng, t) for _ in range(20)] + [_edited(rng, t2) for _ in range(20)]
  reads, starts = _reads(rng, seqs, 's')
  return dict(name='shared_rows', reads=reads, starts=starts, items=[_item(0, seqs, 0), _item(0, seqs, 1, REF_START + 7)],
              targets=[t, t2], cfg=dict(CFG), kinds={})


def large_batch():
  """>= 300 pairs in >= 5 items; the item in the middle (poly-A reads) produces no words: the compaction crosses
  wave (64) and workgroup (256) boundaries with a hole in it."""
  rng = np.random.default_rng(20261022)
  t = _seq(rng, 256)
  targets = [t, t[:120] + 'GT' + t[120:], t[:60] + t[66:], t[:200] + 'C' + t[200:], t[10:250]]
  normal = [_edited(rng, targets[int(rng.integers(0, len(targets)))]) for _ in range(70)]
  poly_a = ['A' * int(rng.integers(8, 60)) for _ in range(70)]
  reads, starts = _reads(rng, normal + poly_a, 'b')
  items = [_item(0, normal, 0), _item(0, normal, 1), _item(70, poly_a, 0), _item(0, normal, 2), _item(0, normal, 3),
           _item(30, normal[30:], 4)]
  return dict(name='large', reads=reads, starts=starts, items=items, targets=targets, cfg=dict(CFG), kinds={})


def default_config_batch():
  """The realigner flags' defaults (make_examples_native.DEFAULT_ALN_CONFIG: gap_extend 2, kmer_size 32)."""
  from deepvariant_amd import make_examples_native as men
  rng = np.random.default_rng(20261023)
  t = _seq(rng, 147, 'ACGT')
  seqs = [_edited(rng, t) for _ in range(40)]
  reads, starts = _reads(rng, seqs, 'd')
  return dict(name='default_config', reads=reads, starts=starts, items=[_item(0, seqs, 0)], targets=[t],
              cfg=dict(men.DEFAULT_ALN_CONFIG), kinds={})


def batches():
  return [kinds_batch(), shared_rows_batch(), large_batch(), default_config_batch()]


def table_of(batch):
  from deepvariant_amd import packing
  return packing.ReadTable.from_reads(batch['reads'], alignment_positions=batch['starts'])


def object_route(batch, normalize_reads=False):
  """fast_pass_aligner.realign_reads_to_haplotype item after item -> per item the list it returns."""
  from deepvariant_amd import fast_pass_aligner as fpa
  cfg = dict(batch['cfg'], normalize_reads=normalize_reads)
  out = []
  for first, n_rows, target, ref_start, _ in batch['items']:
    hap = batch['targets'][target]
    out.append(fpa.realign_reads_to_haplotype(hap, batch['reads'][first:first + n_rows], 'chr1', ref_start,
                                              ref_start + len(hap), Ref(), cfg))
  return out
