"""dv_genotype_sites_device (csrc/genotype.hip) against its host twin on every case of tests/genotype_cases.py, every
array with ==; and the fused route's --vcf_outfile against the host path over the same run's CallVariantsOutput
records."""
import numpy as np
import pytest
import torch

from deepvariant_amd import dv_types as T
from deepvariant_amd import postprocess_variants as pp
from tests import genotype_cases as G

pytestmark = pytest.mark.gpu

CASES = G.cases()
_HOST = {}


def host(name):
  """The host twin's result, computed once per case."""
  if name not in _HOST:
    probs, sites, t = CASES[name]
    _HOST[name] = pp.genotype_sites(probs, *pp.site_tables(sites), t=t)
  return _HOST[name]


def assert_same(got, want):
  for field in ('rounded', 'pred_off', 'predictions', 'best', 'removed', 'status'):
    a, b = getattr(got, field), getattr(want, field)
    assert a.dtype == b.dtype and a.shape == b.shape and (a == b).all(), field


def assert_stats(sites, n_items):
  stats = pp.last_device_stats()
  on_host = G.above_device_limit(sites)
  assert stats['sites'] == len(sites) and stats['sites_on_host'] == on_host
  if on_host < len(sites):
    assert stats['launches'] >= 1 and stats['bytes_down'] > 0
  else:
    assert stats['launches'] == 0         # nothing for the device to do


@pytest.mark.parametrize('memory', ['host', 'device'])
@pytest.mark.parametrize('name', sorted(CASES))
def test_device_equals_host(name, memory):
  probs, sites, t = CASES[name]
  tables = pp.site_tables(sites)
  given = probs if memory == 'host' else torch.from_numpy(probs).cuda()
  assert_same(pp.genotype_sites_device(given, *tables, t=t), host(name))
  assert_stats(sites, probs.shape[0])


def test_on_a_callers_stream():
  probs, sites, t = CASES['mixed_257']
  tables = pp.site_tables(sites)
  stream = torch.cuda.Stream()
  with torch.cuda.stream(stream):
    given = torch.from_numpy(probs).cuda(non_blocking=False)
    got = pp.genotype_sites_device(given, *tables, t=t)          # the tensor's current stream is the caller's
  assert_same(got, host('mixed_257'))
  got = pp.genotype_sites_device(probs, *tables, t=t, stream=stream.cuda_stream)
  assert_same(got, host('mixed_257'))
  assert pp.last_device_stats()['launches'] == 1


def test_a_call_of_sites_above_the_limit_launches_nothing():
  probs, sites, t = CASES['a7']
  assert G.above_device_limit(sites) == len(sites) == 1
  for given in (probs, torch.from_numpy(probs).cuda()):
    assert_same(pp.genotype_sites_device(given, *pp.site_tables(sites), t=t), host('a7'))
    stats = pp.last_device_stats()
    assert (stats['sites'], stats['sites_on_host'], stats['launches']) == (1, 1, 0)
  assert stats['bytes_down'] == probs.nbytes      # the site's probabilities came home for the host code


def test_status_errors_reach_python_from_the_device_route():
  probs, sites, t = CASES['bad_sum_in_a2']
  tables = pp.site_tables(sites)
  given = torch.from_numpy(probs).cuda()
  result = pp.genotype_sites_device(given, *tables, t=t)
  with pytest.raises(ValueError, match='Invalid genotype likelihoods do not sum to one'):
    pp.check_status(result, lambda i: given[i].cpu().numpy(), tables[1], lambda s: 'site')


# ---------------------------------------------------------------------------------------------- the fused route
def _run(argv):
  from deepvariant_amd import make_examples as me
  ap = me.build_arg_parser()
  argv = me.absl_booleans(ap, argv)
  args = ap.parse_args(argv)
  me.apply_flags_for_calling(ap, args, argv)
  return me.make_examples_runner(args)


def test_vcf_from_the_fused_route(tmp_path, monkeypatch):
  """The Illumina golden fixture as test_hip_pipeline.py prepares it (78 sites, 84 images, the seeded model): the VCF
  of the device route equals, byte for byte, the VCF the host path makes from the fused route's CallVariantsOutput
  records, and those records equal the ones the route writes without --vcf_outfile."""
  from deepvariant_amd import genomics_io
  from deepvariant_amd import tfrecord
  from tests import realigner_fixture as RF
  ref, sets = RF.load()
  stretch_start = 9_995_000
  fasta = str(tmp_path / 'ref.fa.gz')
  genomics_io.write_fasta(fasta, [('chr20', 'N' * stretch_start + ref.get_bases('chr20', stretch_start, 10_100_600))])
  bam = str(tmp_path / 'reads.bam')
  genomics_io.write_bam(bam, [('chr20', 10_100_600)], sets['wgs'], sample_name='NA12878')
  common = ['--ref', fasta, '--reads', bam, '--regions', 'chr20:10,000,000-10,010,000', '--sample_name', 'NA12878',
            '--channel_list', ','.join(T.PILEUP_CHANNELS_WITH_INSERT_SIZE), '--checkpoint', 'random:7']
  today = str(tmp_path / 'today.tfrecord.gz')
  _run(common + ['--call_variants_outfile', today])
  beside, vcf = str(tmp_path / 'beside.tfrecord.gz'), str(tmp_path / 'device.vcf')
  stats = _run(common + ['--call_variants_outfile', beside, '--vcf_outfile', vcf])
  records = list(tfrecord.read_tfrecords(today))
  assert len(records) == 84 and list(tfrecord.read_tfrecords(beside)) == records
  device = stats['genotype_device']
  assert stats['n_vcf_records'] == 78 and stats['n_examples'] == 84
  assert device['sites'] - device['sites_on_host'] == 78 and device['sites_on_host'] == 0 and device['launches'] >= 1
  from_records = str(tmp_path / 'host.vcf')
  assert pp.main(['--infile', today, '--ref', fasta, '--outfile', from_records]) == 0
  text = open(vcf, 'rb').read()
  assert text == open(from_records, 'rb').read()
  rows = [line for line in text.decode().splitlines() if not line.startswith('#')]
  assert len(rows) == 78 and text.decode().splitlines()[-79].endswith('\tNA12878')
  # alone, and through the host code (DV_GENOTYPE_HOST=1): the same bytes
  monkeypatch.setenv('DV_GENOTYPE_HOST', '1')
  alone = str(tmp_path / 'alone.vcf.gz')
  stats = _run(common + ['--vcf_outfile', alone])
  import gzip
  assert gzip.open(alone, 'rb').read() == text and stats['genotype_device'] == {} and stats['n_examples'] == 84
  # the Read-object path queues each region by itself: one launch per region with candidates, the same bytes
  monkeypatch.delenv('DV_GENOTYPE_HOST')
  monkeypatch.setenv('DV_REGION_OBJECTS', '1')
  objects = str(tmp_path / 'objects.vcf')
  stats = _run(common + ['--vcf_outfile', objects])
  assert not stats['table_path'] and open(objects, 'rb').read() == text
  assert stats['genotype_device']['sites'] == 78 and stats['genotype_device']['sites_on_host'] == 0
