"""Trimmed and alt-aligned regions through the batched route (DV_PACK_DEVICE=1): a batch of regions with
trim_reads_for_pileup -- alt mode none, diff_channels or base_channels -- is trimmed per region, realigned to its alt
haplotypes by ONE alt_align_table call, packed by one dv_pack_draws_device call and drawn by one encoder launch
(ExamplesGenerator.encode_regions_on_device), and every region gets the bytes and the plan of the per-region route
(encode_region_on_device); the configurations left out keep that route; make_examples writes the same file."""
import dataclasses
import os

import numpy as np
import pytest

from deepvariant_amd import dv_types as T
from deepvariant_amd import packing
from tests.test_hip_alt_align_route import _region

pytestmark = pytest.mark.gpu


def _generator(mode, types, sort_by_support=False, trim=True, **sample):
  from deepvariant_amd import make_examples_native as men
  options, ref, reads, cands = _region(mode, types)
  pic = dataclasses.replace(options.pic_options, sort_by_alt_allele_support=sort_by_support)
  so = dataclasses.replace(options.sample_options[0], **sample)
  options = dataclasses.replace(options, pic_options=pic, sample_options=[so], trim_reads_for_pileup=trim)
  return men.ExamplesGenerator(options, {}, test_mode=True, ref_reader=ref), pic, reads, cands


def _cut(table, cands, cuts):
  """Regions of consecutive candidates, each with the rows its candidates can reach (and a few more)."""
  ends, starts = table.read_end.astype(np.int64), table.read_pos.astype(np.int64)
  regions = []
  for lo, hi in zip(cuts[:-1], cuts[1:]):
    part = cands[lo:hi]
    a, b = min(c.variant.start for c in part) - 150, max(c.variant.end for c in part) + 150
    regions.append((part, table.take(np.nonzero((ends > a) & (starts < b))[0])))
  return regions


def _assert_same_drawing(gen, regions, shape):
  """encode_regions_on_device over `regions` [(candidates, table)] = encode_region_on_device region by region."""
  together = gen.encode_regions_on_device(regions, shape)
  assert len(together) == len(regions)
  n = 0
  for (cands, table), (images, plan) in zip(regions, together):
    want_images, want_plan = gen.encode_region_on_device(cands, [table], [0], [0.0], shape) if cands else (None, [])
    assert plan == want_plan
    if not want_plan:
      assert images is None and want_images is None
      continue
    assert images.shape == want_images.shape and images.dtype == want_images.dtype
    got, want = images.cpu().numpy(), want_images.cpu().numpy()
    assert got.tobytes() == want.tobytes(), 'examples %s differ' % np.nonzero((got != want).reshape(len(plan), -1).any(1))[0][:5]
    n += len(plan)
  return n


@pytest.mark.parametrize('sort_by_support', [False, True])
@pytest.mark.parametrize('mode,types', [('none', 'all'), ('diff_channels', 'all'), ('diff_channels', 'indels'),
                                        ('base_channels', 'indels')])
def test_a_batch_of_trimmed_regions_is_drawn_as_region_by_region(mode, types, sort_by_support, monkeypatch):
  from deepvariant_amd import alt_aligned_pileup_lib as A
  monkeypatch.setenv('DV_ALT_ALIGN_TABLES', '1')
  gen, pic, reads, cands = _generator(mode, types, sort_by_support)
  table = packing.ReadTable.from_reads(reads)
  assert gen.device_pack_ok(table)
  n = len(cands)                                   # the early insertion first: its haplotype is shorter than the window
  regions = _cut(table, cands, [0, 5, 6, n // 2, n])
  regions.insert(2, ([], regions[0][1]))           # ... and a region without candidates
  shape = [pic.height, pic.width, len(pic.channels)]
  calls, packs = [], []
  real, real_pack = A.alt_align_table, packing.pack_draws_device
  monkeypatch.setattr(A, 'alt_align_table', lambda *a, **kw: (calls.append((len(a[1]), kw.get('device'))), real(*a, **kw))[1])
  monkeypatch.setattr(packing, 'pack_draws_device', lambda *a, **kw: (packs.append(len(a[2])), real_pack(*a, **kw))[1])
  together = gen.encode_regions_on_device(regions, shape)
  # one alt-align call for the batch, on the device, over the items of every region; one pack call
  if mode == 'none':
    assert calls == []
  else:
    assert len(calls) == 1 and calls[0][1] is True and calls[0][0] >= 8
  n_examples = sum(len(plan) for _, plan in together)
  assert len(packs) == 1 and packs[0] >= n_examples > n
  if mode != 'none':
    assert packs[0] > n_examples                   # alt draws behind the reference draws
  stats = packing.pack_draws_stats()
  assert stats['draws'] == packs[0] and stats['launches'] == 1 and stats['candidates'] == n
  calls.clear()
  packs.clear()
  assert _assert_same_drawing(gen, regions, shape) == n_examples
  assert len(packs) == 1                           # the per-region route never packs draws
  if mode != 'none':
    assert 3 <= len(calls) <= 1 + 4                # ... and aligns once per region that has items
    # the alt channels carry something
    images = np.concatenate([img.cpu().numpy() for img, plan in together if plan])
    assert images[..., -2:].any()


def test_names_alone_give_the_same_drawing(monkeypatch):
  """Calls that carry support_rows (the device caller's) and calls that carry names only are drawn alike."""
  monkeypatch.setenv('DV_ALT_ALIGN_TABLES', '1')
  gen, pic, reads, cands = _generator('diff_channels', 'indels')
  table = packing.ReadTable.from_reads(reads)
  regions = _cut(table, cands, [0, 9, len(cands)])
  shape = [pic.height, pic.width, len(pic.channels)]
  by_name = gen.encode_regions_on_device(regions, shape)
  for part, region_table in regions:
    row_of = {}
    for row, key in enumerate(region_table.keys):
      row_of.setdefault(key, row)
    for c in part:
      c.support_rows = {alt: np.array([row_of[name] for name in s.read_names if name in row_of], np.int64)
                        for alt, s in c.allele_support.items()}
      c.allele_support = {alt: T.SupportingReads(read_names=[name for name in s.read_names if name in row_of])
                          for alt, s in c.allele_support.items()}
  by_row = gen.encode_regions_on_device(regions, shape)
  for (a, plan_a), (b, plan_b) in zip(by_name, by_row):
    assert plan_a == plan_b and a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


def test_what_is_left_out_keeps_the_per_region_route(monkeypatch):
  monkeypatch.setenv('DV_ALT_ALIGN_TABLES', '1')
  for mode, types, trim, sample in (('rows', 'all', True, {}), ('single_row', 'indels', True, {}),
                                    ('diff_channels', 'indels', False, {}), ('base_channels', 'all', False, {}),
                                    ('diff_channels', 'indels', True, dict(alt_aligned_pileup='rows')),
                                    ('none', 'all', True, dict(use_non_uniform_downsampling=True)),
                                    ('none', 'all', True, dict(channels_enum_to_blank=[3]))):
    gen, pic, _, _ = _generator(mode, types, trim=trim, **sample)
    assert not gen.device_pack_ok(), (mode, types, trim, sample)
    with pytest.raises(ValueError, match='does not qualify'):
      gen.encode_regions_on_device([([], None)], [gen._height, pic.width, len(pic.channels)])   # pylint: disable=protected-access
  # trim-all configurations are taken, with keep_only_window_spanning_reads too; Read objects never are
  for mode, sample in (('none', {}), ('diff_channels', {}), ('base_channels', dict(keep_only_window_spanning_reads=True))):
    gen, _, reads, _ = _generator(mode, 'indels', **sample)
    assert gen.device_pack_ok() and not gen.device_pack_ok(reads)
  # the alt-aligned modes need the table aligner's switch
  monkeypatch.delenv('DV_ALT_ALIGN_TABLES', raising=False)
  assert not _generator('diff_channels', 'indels')[0].device_pack_ok()
  assert _generator('none', 'all')[0].device_pack_ok()


def test_window_spanning_reads_only(monkeypatch):
  """keep_only_window_spanning_reads next to trim_reads_for_pileup: the trimmed lists are shorter, the drawing is
  the per-region route's."""
  monkeypatch.setenv('DV_ALT_ALIGN_TABLES', '1')
  gen, pic, reads, cands = _generator('diff_channels', 'indels', keep_only_window_spanning_reads=True)
  table = packing.ReadTable.from_reads(reads)
  regions = _cut(table, cands, [0, 7, len(cands)])
  assert _assert_same_drawing(gen, regions, [pic.height, pic.width, len(pic.channels)]) > len(cands)


def test_one_pacbio_partition_in_five_regions(monkeypatch):
  """The first 25 kb partition of the PacBio fixture (the golden run's image options minus base_methylation, as
  test_hip_alt_align_route takes it) in five 5 kb regions: HiFi reads, width 147, diff_channels for indels."""
  from deepvariant_amd import make_examples_native as men
  from deepvariant_amd.realigner import utils as U
  from tests import pacbio_chain as PC
  ref, reads, meta, _ = PC.load()
  pic = PC.pic_options(True)
  pic.channels = [c for c in pic.channels if c != 'base_methylation']
  pic.num_channels = len(pic.channels)
  options = T.MakeExamplesOptions(pic_options=pic, trim_reads_for_pileup=True,
                                  sample_options=[T.SampleOptions(role='main', name='s', pileup_height=100)])
  monkeypatch.setenv('DV_ALT_ALIGN_TABLES', '1')
  gen = men.ExamplesGenerator(options, {}, test_mode=True, ref_reader=ref)
  regions, n_cands = [], 0
  for k in range(5):
    region = T.Range('chr20', PC.REGION.start + 5000 * k, PC.REGION.start + 5000 * (k + 1))
    in_reads = [r for r in reads if U.ranges_overlap(U.read_range(r), region)]
    seen, cands = set(), []
    for start, end, refb, alts, _ in meta:
      if region.start <= start < region.end and (start, alts) not in seen:
        seen.add((start, alts))
        cands.append(T.DeepVariantCall(variant=T.Variant('chr20', start, end, refb, list(alts)), allele_support={}))
    regions.append((cands, packing.ReadTable.from_reads(in_reads)))
    n_cands += len(cands)
  assert n_cands > 20 and sum(1 for cands, _ in regions if cands) >= 3
  assert gen.device_pack_ok(regions[0][1])
  assert _assert_same_drawing(gen, regions, [100, 147, 9]) >= n_cands


@pytest.mark.timeout(900)
def test_make_examples_writes_the_same_file_with_the_switch(tmp_path, monkeypatch):
  """make_examples --alt_aligned_pileup diff_channels --types_to_alt_align indels --trim_reads_for_pileup
  --call_variants_outfile --checkpoint random:7 over 20 kb of NA12878, DV_ALT_ALIGN_TABLES=1 in both runs:
  DV_PACK_DEVICE=1 writes the file a run without the switch writes, and only the switched run packs draws."""
  from deepvariant_amd import genomics_io
  from deepvariant_amd import make_examples as me
  from deepvariant_amd import tfrecord
  golden_dir = os.path.join(os.path.dirname(__file__), 'golden')
  with np.load(os.path.join(golden_dir, 'na12878_100kb.npz')) as z:
    bam = str(tmp_path / 'reads.bam')
    with open(bam, 'wb') as f:
      f.write(z['bam'].tobytes())
    with open(bam + '.bai', 'wb') as f:
      f.write(z['bai'].tobytes())
    fasta = str(tmp_path / 'ref.fa')
    genomics_io.write_fasta(fasta, [('chr20', 'N' * int(z['ref_start'][0]) + z['ref_bases'].tobytes().decode())])
  common = ['--ref', fasta, '--reads', bam, '--regions', 'chr20:10,020,000-10,040,000', '--sample_name', 'NA12878',
            '--alt_aligned_pileup', 'diff_channels', '--types_to_alt_align', 'indels', '--trim_reads_for_pileup',
            '--checkpoint', 'random:7']
  packs = []
  real_pack = packing.pack_draws_device
  monkeypatch.setattr(packing, 'pack_draws_device', lambda *a, **kw: (packs.append(len(a[2])), real_pack(*a, **kw))[1])
  monkeypatch.setenv('DV_ALT_ALIGN_TABLES', '1')
  monkeypatch.delenv('DV_PACK_DEVICE', raising=False)
  plain = str(tmp_path / 'plain.cvo.tfrecord.gz')
  assert me.main(common + ['--call_variants_outfile', plain]) == 0
  assert not packs                                                   # the new function is never called
  monkeypatch.setenv('DV_PACK_DEVICE', '1')
  switched = str(tmp_path / 'switched.cvo.tfrecord.gz')
  assert me.main(common + ['--call_variants_outfile', switched]) == 0
  assert packs and max(packs) > 40                                   # batches of regions, one pack call each
  want, got = list(tfrecord.read_tfrecords(plain)), list(tfrecord.read_tfrecords(switched))
  assert got == want and len(want) > 40
