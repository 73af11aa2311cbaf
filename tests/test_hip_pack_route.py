"""The device packer through the product (DV_PACK_DEVICE=1): read support by row from the device caller to the
calls (DeepVariantCall.support_rows), a batch of regions packed by one dv_pack_regions_device call and drawn by one
encoder launch (ExamplesGenerator.encode_regions_on_device) against the per-region route
(encode_region_on_device: dv_pack_region by name, one launch per region), and make_examples' fused route with the
switch set against the same run without it."""
import dataclasses
import os

import numpy as np
import pytest

from deepvariant_amd import dv_types as T
from deepvariant_amd import packing

pytestmark = pytest.mark.gpu


def _na12878(tmp_path):
  from deepvariant_amd import make_examples_core as mec
  from tests import test_hip_gvcf as HG
  from tests.golden.make_golden import wgs_options
  bam, ref = HG._bam_fixture(tmp_path)                              # pylint: disable=protected-access
  regions = list(mec.partition(T.Range('chr20', ref.offset, ref.offset + len(ref.seq)), 1000))
  table = packing.ReadTable.from_bam(bam, 'chr20', regions[0].start, regions[-1].end, min_mapping_quality=5,
                                     keep_supplementary=True)
  options = T.MakeExamplesOptions(pic_options=wgs_options(),
                                  sample_options=[T.SampleOptions(role='main', name='NA12878', pileup_height=100)])
  ends = table.read_end.astype(np.int64)
  # every region's table with a few rows that do not overlap it in front: rows of the counter's table are not
  # rows of the table the region is packed from
  tables = []
  for r in regions:
    rows = np.nonzero((ends > r.start - 400) & (table.read_pos.astype(np.int64) < r.end))[0]
    tables.append(table.take(rows))
  proc = mec.RegionProcessor(options, ref, mec.RegionProcessorOptions(realigner_enabled=False))
  return proc, regions, tables


def _assert_same_drawing(gen, regions, shape):
  """encode_regions_on_device over `regions` [(candidates, table)] = encode_region_on_device region by region."""
  together = gen.encode_regions_on_device(regions, shape)
  assert len(together) == len(regions)
  n = 0
  for (cands, table), (images, plan) in zip(regions, together):
    want_images, want_plan = gen.encode_region_on_device(cands, [table], [0], [0.0], shape)
    assert plan == want_plan
    if not want_plan:
      assert images is None and want_images is None
      continue
    assert images.shape == want_images.shape and images.dtype == want_images.dtype
    assert images.cpu().numpy().tobytes() == want_images.cpu().numpy().tobytes()
    n += len(plan)
  return n


def test_support_rows_name_the_reads_allele_support_names(tmp_path, monkeypatch):
  proc, regions, tables = _na12878(tmp_path)
  called = proc.process_tables(regions, tables)
  n_calls = n_rows = n_shifted = 0
  for (cands, realigned), region in zip(called, regions):
    keys = realigned.keys
    for call in cands:
      assert call.support_rows is not None and list(call.support_rows) == list(call.allele_support)
      for alt, support in call.allele_support.items():
        rows = call.support_rows[alt]
        assert [keys[r] for r in rows.tolist()] == support.read_names
        n_rows += len(rows)
      n_calls += 1
    n_shifted += int(bool(cands) and realigned.read_end[0] <= region.start)      # row 0 is not the counter's row 0
  assert n_calls >= 149 and n_rows > 1000 and n_shifted > 10
  # ... and a batch of those regions is drawn as region by region, support taken by row
  shape = [100, proc.options.pic_options.width, len(proc.options.pic_options.channels)]
  with_cands = [(c, t) for c, t in called if c][:24] + [([], called[0][1])]
  calls = []
  real = packing.support_arrays
  monkeypatch.setattr(packing, 'support_arrays', lambda table, cands: (
      calls.append(all(c.support_rows is not None for c in cands)), real(table, cands))[1])
  assert _assert_same_drawing(proc.generator, with_cands, shape) > 30
  assert calls and all(calls)
  # a call that carries names only gives the same drawing
  for cands, _ in with_cands:
    for c in cands:
      c.support_rows = None
  assert _assert_same_drawing(proc.generator, with_cands, shape) > 30


@pytest.mark.parametrize('sort_by_support', [False, True])
def test_a_batch_of_synthetic_regions_is_drawn_as_region_by_region(sort_by_support, monkeypatch):
  from deepvariant_amd import make_examples_native as men
  from deepvariant_amd import synth
  opts = dataclasses.replace(synth.illumina_options(7), sort_by_alt_allele_support=sort_by_support)
  base = synth.make_illumina_batch(90, seed=13, options=opts)
  table, cands, combos, windows = synth.region_inputs_from_batch(base, opts)
  window_of = {id(c.variant): w for c, w in zip(cands, windows)}
  monkeypatch.setattr(men, 'get_reference_bases_for_pileup',
                      lambda ref, variant, width: window_of[id(variant)])
  options = T.MakeExamplesOptions(pic_options=opts,
                                  sample_options=[T.SampleOptions(role='main', pileup_height=opts.height)])
  gen = men.ExamplesGenerator(options, {}, test_mode=True, ref_reader=object())
  assert gen.device_pack_ok(table)
  # four regions of candidates, each with the rows its candidates can pick (and the last with none: empty)
  ends, starts = table.read_end.astype(np.int64), table.read_pos.astype(np.int64)
  regions = []
  for part in (cands[:31], cands[31:32], cands[32:70], cands[70:]):
    lo, hi = min(c.variant.start for c in part) - 50, max(c.variant.end for c in part) + 50
    regions.append((part, table.take(np.nonzero((ends > lo) & (starts < hi))[0])))
  regions.insert(2, ([], regions[0][1]))
  shape = [opts.height, opts.width, 7]
  assert _assert_same_drawing(gen, regions, shape) == base.n_items
  stats = packing.pack_device_stats()
  assert stats['regions'] == 5 and stats['candidates'] == len(cands) and stats['items'] == base.n_items
  assert stats['launches'] == 3


def test_the_golden_slice_in_two_regions():
  from deepvariant_amd import make_examples_native as men
  from tests import golden_io
  from tests.golden.make_golden import wgs_options
  from tests.test_oracle_golden import FIXTURE
  from tests.test_hip_pipeline import _WindowRef
  reads, examples, _ = golden_io.load(FIXTURE)
  pic = wgs_options()
  options = T.MakeExamplesOptions(pic_options=pic, sample_options=[T.SampleOptions(role='main', pileup_height=100)])
  cands, seen = [], set()
  for ex in examples:
    key = (ex['call'].variant.start, tuple(ex['call'].variant.alternate_bases))
    if key not in seen:
      seen.add(key)
      cands.append(ex['call'])
  gen = men.ExamplesGenerator(options, {}, test_mode=True, ref_reader=_WindowRef(examples, pic.width))
  table = packing.ReadTable.from_reads(reads)
  half = len(cands) // 2
  shape = [100, pic.width, len(pic.channels)]
  assert _assert_same_drawing(gen, [(cands[:half], table), (cands[half:], table)], shape) == 84
  assert _assert_same_drawing(gen, [(cands, table)], shape) == 84


def test_a_region_that_does_not_qualify_keeps_the_per_region_route():
  from deepvariant_amd import make_examples_native as men
  from deepvariant_amd import synth
  opts = synth.illumina_options(7)
  for so, pic in ((T.SampleOptions(role='main', pileup_height=100, channels_enum_to_blank=[3]), opts),
                  (T.SampleOptions(role='main', pileup_height=100, use_non_uniform_downsampling=True), opts),
                  (T.SampleOptions(role='main', pileup_height=100, keep_only_window_spanning_reads=True), opts),
                  (T.SampleOptions(role='main', pileup_height=100),
                   dataclasses.replace(opts, channels=list(opts.channels[:6]) + ['allele_frequency']))):
    gen = men.ExamplesGenerator(T.MakeExamplesOptions(pic_options=pic, sample_options=[so]), {}, test_mode=True,
                                ref_reader=object())
    assert not gen.device_pack_ok()
    with pytest.raises(ValueError, match='does not qualify'):
      gen.encode_regions_on_device([([], None)], [pic.height, pic.width, len(pic.channels)])
  plain = men.ExamplesGenerator(T.MakeExamplesOptions(pic_options=opts, sample_options=[T.SampleOptions(role='main', pileup_height=100)]),
                                {}, test_mode=True, ref_reader=object())
  assert plain.device_pack_ok() and not plain.device_pack_ok([])          # Read objects: the per-region route


@pytest.mark.timeout(900)
def test_make_examples_writes_the_same_file_with_the_switch(tmp_path, monkeypatch):
  """make_examples --call_variants_outfile --checkpoint random:7 over 20 kb of NA12878: DV_PACK_DEVICE=1 writes the
  file a run without the switch writes, and only the switched run calls pack_regions_device."""
  from deepvariant_amd import genomics_io
  from deepvariant_amd import make_examples as me
  from deepvariant_amd import make_examples_core as mec
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
            '--channel_list', ','.join(T.PILEUP_CHANNELS_WITH_INSERT_SIZE), '--checkpoint', 'random:7']
  packs, batches = [], []
  real_pack = packing.pack_regions_device
  real_queue = mec.RegionProcessor.queue_regions_candidates
  monkeypatch.setattr(packing, 'pack_regions_device', lambda *a, **kw: (packs.append(len(a[0])), real_pack(*a, **kw))[1])
  monkeypatch.setattr(mec.RegionProcessor, 'queue_regions_candidates',
                      lambda self, called, model: (batches.append(len(called)), real_queue(self, called, model))[1])
  monkeypatch.delenv('DV_PACK_DEVICE', raising=False)
  plain = str(tmp_path / 'plain.cvo.tfrecord.gz')
  assert me.main(common + ['--call_variants_outfile', plain]) == 0
  assert not packs and not batches                                   # the new functions are never called
  monkeypatch.setenv('DV_PACK_DEVICE', '1')
  switched = str(tmp_path / 'switched.cvo.tfrecord.gz')
  assert me.main(common + ['--call_variants_outfile', switched]) == 0
  assert packs and max(packs) > 1 and sum(batches) >= 20             # batches of regions, one pack call each
  want, got = list(tfrecord.read_tfrecords(plain)), list(tfrecord.read_tfrecords(switched))
  assert got == want and len(want) > 40
