"""The Illumina golden chain of tests/test_hip_realigner.py through the table path with the realigner's local
alignments on the device: run as a program (python -m tests.realign_device_chain) in a process of its own, so
that DV_REALIGN_DEVICE=1 is read the way make_examples reads it.  Raw reads of chr20:10,000,000-10,010,000 ->
Realigner.realign_tables (dv_realign_regions_device) -> dv_count_alleles -> candidate caller ->
dv_encode_batch: all 84 golden images, bit for bit.  Exit status 0 and a line "84/84" on success."""
import os
import sys

import numpy as np


def main():
  from deepvariant_amd import dv_types as T
  from deepvariant_amd import make_examples_core as mec
  from deepvariant_amd import packing
  from deepvariant_amd import protowire as pw
  from deepvariant_amd.realigner import realigner as R
  from deepvariant_amd.realigner import utils as U
  from tests import golden_io
  from tests import realigner_fixture as RF
  from tests.golden.make_golden import wgs_options
  assert os.environ.get('DV_REALIGN_DEVICE') == '1' and R._DEVICE_ALIGN      # pylint: disable=protected-access
  ref, sets = RF.load()
  _, examples, _ = golden_io.load(os.path.join(os.path.dirname(__file__), 'golden', 'illumina_wgs_chr20.npz'))
  options = T.MakeExamplesOptions(pic_options=wgs_options(),
                                  sample_options=[T.SampleOptions(role='main', name='NA12878', pileup_height=100)])
  proc = mec.RegionProcessor(options, ref)
  assert proc.realigner.device_align
  # every realigner call of the chain must have gone to the device
  calls = []
  run = R.RealignJob._call                                                   # pylint: disable=protected-access

  def counted(job):
    out = run(job)
    calls.append(job.device_stats)
    return out
  R.RealignJob._call = counted                                               # pylint: disable=protected-access
  reads = sets['wgs']
  spans = [U.read_range(r) for r in reads]
  images = {}
  for region in mec.partition(T.Range('chr20', 9_999_999, 10_010_000), 1000):
    table = packing.ReadTable.from_reads([r for r, s in zip(reads, spans) if U.ranges_overlap(s, region)])
    _, encoded = proc.examples_in_region_table(region, table)
    for blob in encoded:
      ex = pw.decode_example(blob)
      v = pw.decode_variant(ex['variant/encoded'][0])
      alts = tuple(v.alternate_bases[i] for i in pw.decode_alt_allele_indices(ex['alt_allele_indices/encoded'][0]))
      images[(v.start, alts)] = np.frombuffer(ex['image/encoded'][0], np.uint8).reshape(ex['image/shape'])
  assert calls and all(s is not None for s in calls), 'the realigner did not take the device route'
  assert sum(s.pairs for s in calls) > 0 and sum(s.pairs_on_host for s in calls) == 0
  assert len(images) == len(examples) == 84, len(images)
  good = sum(int(np.array_equal(images[(ex['call'].variant.start, tuple(ex['alt_alleles']))], ex['image']))
             for ex in examples)
  print('%d/%d' % (good, len(examples)))
  return 0 if good == len(examples) else 1


if __name__ == '__main__':
  sys.exit(main())
