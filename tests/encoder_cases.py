"""Pileup inputs that steer the HIP encoder's phase D (deepvariant_amd/csrc/encoder.hip) down a chosen route: reads with
an EXACT number of CIGAR operations (the LDS cache holds 8 / 16 / 32 / 64 words per read, longer CIGARs come from
global memory in chunks of 64 operations), placed so that a chosen operation lies on a chosen column, in windows that
are filled across their whole width (a row is rendered in passes of 256 columns).  Inputs only: tests/
test_encoder_cases_cpu.py proves with the oracle alone that the cases are what they claim, tests/
test_hip_encoder_paths.py feeds them to the kernel.  Built on tests/fuzz_inputs.py (options, op codes)."""
import dataclasses
import zlib

import numpy as np

from deepvariant_amd import dv_types as T
from deepvariant_amd import packing
from tests import fuzz_inputs as F

KINDS = 'MIDNSHP=X'                 # all nine operation kinds
M_KINDS = 'M=X'                     # the kinds that draw aligned bases
_REF_OPS = (1, 3, 4, 8, 9)          # consume the reference: M D N = X
_QUERY_OPS = (1, 2, 5, 8, 9)        # consume the read: M I S = X
# aligned kinds three times as likely as each other kind: about half of a read's operations draw bases
_WEIGHTED = 'MMM===XXXIDNSHP'
MIN_BQ, MIN_MAPQ = 10, 5            # fuzz_inputs.options' read requirements

# ---- the shapes of tests/test_hip_encoder_paths.py (here so that the CPU test can check every one of them)
OP_COUNTS = (7, 8, 9, 15, 16, 17, 63, 64, 65, 127, 128, 129, 200)
BOUNDARY_WIDTHS = (61, 221)
PASS_WIDTHS = (255, 257, 301, 511, 513)       # 1, 2, 2, 2, 3 passes of 256 columns
CHANNELS_16 = ['read_base', 'base_quality', 'mapping_quality', 'strand', 'read_supports_variant',
               'base_differs_from_ref', 'haplotype', 'read_mapping_percent', 'avg_base_quality', 'identity',
               'gap_compressed_identity', 'gc_content', 'is_homopolymer', 'homopolymer_weighted', 'insert_size',
               'supplementary_alignment']
# (name, channel list, out_channels): dv_encode_batch pads every pixel to out_channels bytes
PADDED = [('c7', T.PILEUP_CHANNELS_WITH_INSERT_SIZE, oc) for oc in (7, 8, 9, 12, 16, 17, 20, 33, 64)] + \
         [('c16', CHANNELS_16, oc) for oc in (16, 18)] + \
         [('c6', T.PILEUP_DEFAULT_CHANNELS, oc) for oc in (6, 8)]


def padded_widths(out_channels):
  return (61,) if out_channels > 16 else (61, 221)


def seed_of(name):
  return zlib.crc32(name.encode())   # (str hashes differ per process)


def exact_cigar(rng, n_ops, pins=None):
  """Exactly `n_ops` CigarUnits with lengths 1-4, no two neighbours of the same kind (nothing can merge them), drawn
  from all nine kinds.  `pins`: {index: (kinds, length | None)} fixes the kind (one of `kinds`) and length of chosen
  operations; the last operation draws aligned bases unless pinned otherwise, so the read is never empty."""
  pins = dict(pins or {})
  pins.setdefault(n_ops - 1, (M_KINDS, None))
  ops, prev = [], ''
  for k in range(n_ops):
    kinds, length = pins.get(k, (_WEIGHTED, None))
    nxt = pins[k + 1][0] if k + 1 in pins else ''
    # a pinned neighbour of ONE possible kind must stay different from this operation
    pool = [c for c in kinds if c != prev and not (len(set(nxt)) == 1 and c == nxt[0])]
    op = pool[int(rng.integers(0, len(pool)))]
    ops.append(T.CigarUnit(F._OPS[op], int(length or rng.integers(1, 5))))
    prev = op
  return ops


def ref_offset(cigar, idx):
  return sum(c.operation_length for c in cigar[:idx] if c.operation in _REF_OPS)


def query_offset(cigar, idx):
  return sum(c.operation_length for c in cigar[:idx] if c.operation in _QUERY_OPS)


def last_chunk_index(rng, n_ops):
  """A random operation index inside the read's LAST chunk of 64 operations (the whole read below 65)."""
  return int(rng.integers(64 * ((n_ops - 1) // 64), n_ops))


def reads_with_ops(rng, width, n_ops, n_reads=1, image_start=0, at=None, pins=None, qual_lo=0, mapq=None,
                   with_hp=False, with_mods=False, n_names=None):
  """Proto-shaped reads whose CIGARs have exactly `n_ops` operations (an int, or one count per read) after packing.
  `at`: per read (operation index, column) -- the read starts where that operation begins on that column of the window
  at `image_start` -- or None: a random operation (every other time one of the read's last chunk of 64) on a random
  column, so reads cover the window's whole width.  Qualities are qual_lo..59, mapping qualities 0..69 unless given."""
  counts = [int(n_ops)] * n_reads if np.isscalar(n_ops) else [int(n) for n in n_ops]
  reads = []
  for i, n in enumerate(counts):
    pin = dict((pins[i] if isinstance(pins, list) else pins) or {})
    where = at[i] if at is not None and at[i] is not None else None
    if where is None:
      idx = last_chunk_index(rng, n) if rng.random() < 0.5 else int(rng.integers(0, n))
      where = (idx, int(rng.integers(0, width)))
    cigar = exact_cigar(rng, n, pin)
    qlen = F.query_len(cigar)
    start = image_start + where[1] - ref_offset(cigar, where[0])
    quals = rng.integers(qual_lo, 60, size=qlen).astype(np.uint8)
    r = T.Read(
        fragment_name='frag%d' % int(rng.integers(0, n_names or max(len(counts) // 2, 1))),
        read_number=int(rng.integers(0, 2)), number_reads=2,
        fragment_length=int(rng.integers(-1500, 1500)),
        aligned_sequence=''.join('ACGT'[int(j)] for j in rng.integers(0, 4, size=qlen)),
        aligned_quality=bytes(quals),
        supplementary_alignment=bool(rng.integers(0, 2)),
        alignment=T.LinearAlignment(
            position=T.Position('chr1', start, bool(rng.integers(0, 2))),
            mapping_quality=int(rng.integers(0, 70)) if mapq is None else mapq, cigar=cigar))
    if with_hp and rng.random() < 0.7:
      r.info['HP'] = T.ListValue(values=[T.Value(int_value=int(rng.integers(0, 4)))])
    if with_mods and rng.random() < 0.5:
      r.base_modifications[T.K5MC] = bytes(rng.integers(0, 256, size=qlen).astype(np.uint8))
    if with_mods and rng.random() < 0.5:
      r.base_modifications[T.K6MA] = bytes(rng.integers(0, 256, size=qlen).astype(np.uint8))
    reads.append(r)
  return reads


def _set_quality(read, op_index, value):
  """The quality of the first base of operation `op_index`."""
  q = bytearray(read.aligned_quality)
  q[query_offset(read.alignment.cigar, op_index)] = value
  read.aligned_quality = bytes(q)


def window_case(rng, width, ops, variant_start=1000, with_hp=False, with_mods=False, n_alts=2):
  """(call, ref_window, reads, image_start, alt combo) like fuzz_inputs.make_case, of reads_with_ops reads; `ops`: one
  operation count per read (at least 6 reads).  The first reads are placed by hand, each on an operation of its last
  chunk of 64, with mapping quality 60:
    0     a 4-base aligned operation starts on the variant column with base quality 3: the site gate rejects the read
          (below 65 operations the gate finds the base in the first chunk, above it only by walking the whole CIGAR);
    1     the same with quality 40, every other quality >= 10: accepted;
    2     an insertion whose anchor falls on the LAST column (the operation starts one column past the window);
    3, 4  4-base aligned operations over columns 252-255 | 256 and 508-511 | 512: they span the 256-column pass
          boundaries (wider windows only; narrower ones get random reads instead);
  the others start anywhere, so the window is covered across its whole width."""
  assert width % 2 == 1 and len(ops) >= 6
  hw = (width - 1) // 2
  image_start = variant_start - hw
  ref_window = ''.join('ACGTN'[int(i)] for i in rng.choice(5, size=width, p=[.24, .24, .24, .24, .04]))
  n_names = max(len(ops) // 2, 1)
  kw = dict(image_start=image_start, with_hp=with_hp, with_mods=with_mods, n_names=n_names)
  reads = []
  for i, n in enumerate(ops[:5]):
    idx = last_chunk_index(rng, n)
    if i == 2:
      hand = dict(at=[(idx, width)], pins={idx: ('I', None)}, qual_lo=MIN_BQ, mapq=60)
    elif i in (0, 1):
      hand = dict(at=[(idx, hw)], pins={idx: (M_KINDS, 4)}, qual_lo=MIN_BQ, mapq=60)
    elif 256 * (i - 2) < width:
      hand = dict(at=[(idx, 256 * (i - 2) - 3)], pins={idx: (M_KINDS, 4)}, qual_lo=MIN_BQ, mapq=60)
    else:
      hand = {}
    r = reads_with_ops(rng, width, n, **hand, **kw)[0]
    if i in (0, 1):
      _set_quality(r, idx, 3 if i == 0 else 40)
    reads.append(r)
  reads += reads_with_ops(rng, width, list(ops[5:]), **kw)
  n_reads = len(reads)
  alts = ['C', 'G', 'T'][:n_alts]
  keys = ['%s/%d' % (r.fragment_name, r.read_number) for r in reads]
  support = {a: T.SupportingReads([keys[int(j)] for j in
                                   rng.integers(0, n_reads, size=int(rng.integers(0, n_names + 1)))]) for a in alts}
  call = T.DeepVariantCall(variant=T.Variant('chr1', variant_start, variant_start + 1, 'A', alts),
                           allele_support=support)
  combo = [alts[int(j)] for j in sorted(set(rng.integers(0, n_alts, size=int(rng.integers(1, 3))).tolist()))]
  return call, ref_window, reads, image_start, combo


def cut_reads(reads, n_ops):
  """The same reads with their CIGARs cut after the first `n_ops` operations (sequences unchanged)."""
  out = []
  for r in reads:
    a = r.alignment
    out.append(dataclasses.replace(r, alignment=T.LinearAlignment(
        position=a.position, mapping_quality=a.mapping_quality, cigar=list(a.cigar[:n_ops]))))
  return out


def one_long(n_reads, n_long, at=1):
  """Operation counts of an item of 8-operation reads with ONE read of `n_long` operations (reads 1 and 2 are always
  accepted)."""
  ops = [8] * n_reads
  ops[at] = n_long
  return ops


# ---- one packed batch whose items take both routes
MIXED_WIDTH, MIXED_HEIGHT = 221, 30
MIXED_LONG_OPS = (17, 32, 33, 64, 65, 129, 200)    # 32 | 33 and 64 | 65: the cache sizes of the DV_CIG_CACHE knob


def mixed_batch(seed=seed_of('mixed_batch'), n_items=10, out_channels=7):
  """-> (options, PackedBatch): items over one read table (built the way tests/test_hip_golden.py builds its batch).
  Even items list reads of 1-16 operations only (every CIGAR fits the 16-word cache of a batch whose longest read has
  more: the pipelined route); odd items list the same reads plus reads of MIXED_LONG_OPS operations (the plain route).
  One item has more reads than rows, one a blanked channel."""
  rng = np.random.default_rng(seed)
  w, h = MIXED_WIDTH, MIXED_HEIGHT
  opts = F.options(T.PILEUP_CHANNELS_WITH_INSERT_SIZE, w, h)
  hw = (w - 1) // 2
  short_ops = [int(rng.integers(1, 17)) for _ in range(34)] + [8, 9, 15, 16]
  call, _, short, image_start, combo = window_case(rng, w, short_ops)
  long_reads = window_case(rng, w, list(MIXED_LONG_OPS) * 2)[2]
  reads = short + long_reads
  table = packing.ReadTable.from_reads(reads)
  batch = packing.PackedBatch(table=table, width=w)
  n_short = len(short)
  for i in range(n_items):
    vstart = call.variant.start + 3 * (i // 2) - 6     # neighbouring sites: shared reads land on other columns
    item_call = dataclasses.replace(call, variant=dataclasses.replace(call.variant, start=vstart, end=vstart + 1))
    ref = ''.join('ACGT'[int(j)] for j in rng.integers(0, 4, size=w))
    pick = rng.permutation(n_short)[:n_short if i == 4 else 18]      # item 4: 38 reads for 25 rows (the shuffle)
    if i % 2:
      pick = np.concatenate([pick[:12], n_short + rng.permutation(len(long_reads))[:8]])
      rng.shuffle(pick)
    idx = pick.astype(np.uint32)
    batch.add_item(vstart, vstart - hw, batch.add_ref_window(ref), idx,
                   packing.support_codes(item_call, combo, table, idx), height=h,
                   out_off=i * h * w * out_channels, blank_mask=(1 << 2) if i in (6, 7) else 0)
  return opts, batch


# ---- the kernel's LDS request (dv_encode_batch, encoder.hip): the shapes of the GPU tests stay below 48 KiB
ENC_CONST_BYTES = 4 * 256 + 1008 + 16 + 4 * 16 + 12 * 4


def cig_cache_words(max_ops, kept_cap):
  if max_ops == 0:
    return 8
  cache = 8
  while cache < 16 and cache < max_ops:
    cache *= 2
  while cache > 8 and cache * kept_cap * 4 > 24 * 1024:
    cache //= 2
  return cache


def lds_bytes(width, out_channels, n_channels, height, band, max_ops=200, cig_cache=None, kept_cap=None):
  if kept_cap is None:
    kept_cap = (min(256, height - band) + 3) & ~3
  if cig_cache is None:
    cig_cache = cig_cache_words(max_ops, kept_cap)
  row_buf = (width * out_channels + 16 + 15) & ~15
  return (ENC_CONST_BYTES + 6 * 256 * 4 + 8 * 4 + 3 * kept_cap * ((n_channels + 3) // 4) * 4 +
          kept_cap * cig_cache * 4 + 4 * row_buf)


# ---- the cases of the GPU tests
@dataclasses.dataclass
class Case:
  name: str
  channels: list
  width: int
  height: int
  ops: list                    # CIGAR operations of every read
  okw: dict = dataclasses.field(default_factory=dict)     # options
  ckw: dict = dataclasses.field(default_factory=dict)     # window_case
  blank: str = ''              # channel to blank
  mean_coverage: float = 0.0

  @property
  def max_ops(self):
    return max(self.ops)

  def options(self):
    return F.options(self.channels, self.width, self.height, **dict(self.okw))

  def build(self):
    """-> (call, ref_window, reads, image_start, alt combo), the same for every caller."""
    return window_case(np.random.default_rng(seed_of(self.name)), self.width, self.ops, **self.ckw)

  def blank_enums(self):
    return [int(T.CHANNEL_STR_TO_ENUM[self.blank])] if self.blank else None


_PACBIO = next(c for c in F.CONFIGS if c[0] == 'pacbio_like')
MEAN_COVERAGE_7 = T.PILEUP_DEFAULT_CHANNELS + ['mean_coverage']
BOUNDARY_HEIGHT = 24           # 19 read rows under a band of 5
ONE_LONG = (9, 17, 65, 129, 200)


def boundary_cases(width):
  """(a): every read of an item has exactly n operations, n on both sides of every cache size and chunk end; then
  items of 8-operation reads with ONE long read.  Per count: 14 reads; 30 reads for 19 rows (the shuffle) with a
  blanked channel; 8 reads with mean_coverage painted 6 rows below them; and the same on the 10-channel long-read list
  (haplotype sorting, methylation)."""
  h = BOUNDARY_HEIGHT
  wgs, pb = T.PILEUP_CHANNELS_WITH_INSERT_SIZE, _PACBIO[1]
  pb_okw, pb_ckw = dict(_PACBIO[4]), dict(_PACBIO[5])
  cases = []
  # (of 30 reads the shuffle keeps read 2 whatever the others do: it is accepted and comes first in the permutation)
  for label, ops_of in [('all%d' % n, lambda k, n=n: [n] * k) for n in OP_COUNTS] + \
                       [('one%d' % n, lambda k, n=n: one_long(k, n, at=2 if k == 30 else 1)) for n in ONE_LONG]:
    tag = 'w%d_%s' % (width, label)
    cases += [
        Case(tag + '_wgs7', wgs, width, h, ops_of(14)),
        Case(tag + '_wgs7_deep_blank', wgs, width, h, ops_of(30), blank='base_quality'),
        Case(tag + '_mean_coverage', MEAN_COVERAGE_7, width, h, ops_of(8), mean_coverage=14.0),
        Case(tag + '_pacbio', pb, width, h, ops_of(14), okw=pb_okw, ckw=pb_ckw),
        Case(tag + '_pacbio_deep_blank', pb, width, h, ops_of(30), okw=pb_okw, ckw=pb_ckw, blank='base_methylation'),
    ]
  return cases


def pass_cases(width):
  """(c): windows of 1, 2 or 3 column passes, with CIGARs of up to 8 operations only (the width alone selects the
  plain route) and with long ones among them, under a reference band of 5 and of 2.  Fewer reads than rows."""
  rng = np.random.default_rng(seed_of('pass_cases%d' % width))
  short = [int(rng.integers(1, 9)) for _ in range(28)]
  long_ = [8, 65, 200, 129, 17, 64] + [int(rng.choice([8, 16, 17, 65, 129, 200])) for _ in range(22)]
  cases = []
  for kind, ops in (('short', short), ('long', long_)):
    for band, h in ((5, 40), (2, 32)):
      cases.append(Case('w%d_%s_band%d' % (width, kind, band), T.PILEUP_CHANNELS_WITH_INSERT_SIZE, width, h, list(ops),
                        okw=dict(reference_band_height=band)))
  return cases


def padded_case(name, channels, width):
  """(d): a small window over the channel list, a long read among its reads (both routes pad)."""
  ckw = dict(with_hp=True) if 'haplotype' in channels else {}
  return Case('padded_%s_w%d' % (name, width), list(channels), width, 20, [8, 70] + [8] * 8 + [20, 3], ckw=ckw)
