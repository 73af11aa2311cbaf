"""make_examples --gvcf_outfile: what check_flags accepts and refuses, and what the flags turn on
(DESIGN.md section 22).  No GPU."""
import pytest

from deepvariant_amd import make_examples as me


def parse(extra):
  ap = me.build_arg_parser()
  argv = me.absl_booleans(ap, ['--ref', 'r.fa', '--reads', 'r.bam'] + extra)
  return ap.parse_args(argv)


def check(extra):
  me.check_flags(parse(extra))


def test_accepted_alone_and_beside_the_other_outputs():
  check(['--gvcf_outfile', 'x.g.vcf', '--checkpoint', 'random:1'])
  check(['--gvcf_outfile', 'x.g.vcf.gz', '--checkpoint', 'random:1', '--vcf_outfile', 'x.vcf.gz'])
  check(['--gvcf_outfile', 'x.g.vcf', '--checkpoint', 'random:1', '--call_variants_outfile', 'cvo.tfrecord.gz'])
  check(['--gvcf_outfile', 'x.g.vcf', '--checkpoint', 'random:1', '--vcf_outfile', 'x.vcf',
         '--call_variants_outfile', 'cvo.tfrecord.gz', '--gvcf_gq_binsize', '3', '--include_med_dp'])


def test_refused():
  with pytest.raises(ValueError, match='--gvcf_outfile needs --checkpoint'):
    check(['--gvcf_outfile', 'x.g.vcf'])
  with pytest.raises(ValueError, match='two routes'):
    check(['--gvcf_outfile', 'x.g.vcf', '--checkpoint', 'random:1', '--examples', 'e.tfrecord.gz'])
  with pytest.raises(ValueError, match='--gvcf_outfile runs on one rank'):
    check(['--gvcf_outfile', 'x.g.vcf', '--checkpoint', 'random:1', '--gpus', '2', '--call_variants_outfile', 'c@2.gz'])
  with pytest.raises(ValueError, match='--gvcf_outfile runs on one rank'):
    check(['--gvcf_outfile', 'x.g.vcf', '--checkpoint', 'random:1', '--ranks_per_gpu', '2',
           '--call_variants_outfile', 'c@2.gz'])
  with pytest.raises(ValueError, match='--gvcf_gq_binsize must be positive'):
    check(['--gvcf_outfile', 'x.g.vcf', '--checkpoint', 'random:1', '--gvcf_gq_binsize', '0'])
  # the TFRecord output of the reference's make_examples stays refused, also beside the new flag
  with pytest.raises(ValueError, match='--gvcf is not supported'):
    check(['--gvcf_outfile', 'x.g.vcf', '--checkpoint', 'random:1', '--gvcf', 'g.tfrecord.gz'])
  # nothing to write at all
  with pytest.raises(ValueError, match='is required'):
    check(['--checkpoint', 'random:1'])


def test_the_flags_reach_the_region_processor():
  _, po = me.options_from_flags(parse(['--gvcf_outfile', 'x.g.vcf', '--checkpoint', 'random:1']))
  assert po.gvcf and po.gvcf_arrays_only and po.gvcf_gq_binsize == 5 and not po.include_med_dp
  _, po = me.options_from_flags(parse(['--gvcf_outfile', 'x.g.vcf', '--checkpoint', 'random:1', '--gvcf_gq_binsize', '3',
                                       '--include_med_dp']))
  assert po.gvcf and po.gvcf_gq_binsize == 3 and po.include_med_dp
  _, po = me.options_from_flags(parse(['--vcf_outfile', 'x.vcf', '--checkpoint', 'random:1']))
  assert not po.gvcf and not po.gvcf_arrays_only
