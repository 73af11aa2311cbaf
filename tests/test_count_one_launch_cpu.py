"""The one-launch counting switch without a GPU (DV_COUNT_ONE_LAUNCH, dv_count_batch_last_stats, include/dvhip.h):
the symbol exists, the stats struct's layout matches the ctypes mirror, a null pointer is refused, the switch is off
by default, the batch plan's two new sections hold against tools/count_batch_layout_check.cpp, and the case module
of the GPU tests (tests/count_launch_cases.py) holds the workgroup counts it promises."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from deepvariant_amd import _lib
from deepvariant_amd import allelecounter as A
from deepvariant_amd import packing
from tests import count_launch_cases as L

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
HEADER = os.path.join(ROOT, 'include', 'dvhip.h')


def test_symbols_and_version():
  lib = _lib.lib()
  assert lib.dv_count_batch_last_stats is not None and 'dv_count_batch_last_stats' in _lib.ABI_SYMBOLS
  assert lib.dv_abi_version() == 8
  with open(HEADER) as f:
    header = f.read()
  assert re.search(r'#define DV_ABI_VERSION 8\b', header)
  assert re.search(r'\bint dv_count_batch_last_stats\(dv_count_batch_stats\* out\);', header)
  assert 'DV_COUNT_ONE_LAUNCH' in header


def test_struct_layout():
  s = _lib.DvCountBatchStats
  assert C.sizeof(s) == 24
  assert [(getattr(s, name).offset, getattr(s, name).size) for name, _ in s._fields_] == \
      [(0, 4), (4, 4), (8, 4), (12, 4), (16, 8)]                            # pylint: disable=protected-access
  with open(HEADER) as f:
    body = re.search(r'typedef struct dv_count_batch_stats \{(.*?)\} dv_count_batch_stats;', f.read(), re.S).group(1)
  declared = re.findall(r'^\s*(int32_t|int64_t) (\w+);', body, re.M)
  assert declared == [('int32_t', 'regions'), ('int32_t', 'regions_batched'), ('int32_t', 'regions_alone'),
                      ('int32_t', 'count_launches'), ('int64_t', 'count_workgroups')]
  assert [name for name, _ in s._fields_] == [name for _, name in declared]  # pylint: disable=protected-access


def test_null_pointer_is_refused():
  lib = _lib.lib()
  assert lib.dv_count_batch_last_stats(None) == _lib.DV_ERR_INVALID_ARGUMENT
  assert 'dv_count_batch_last_stats' in lib.dv_last_error().decode()
  stats = _lib.DvCountBatchStats()
  assert lib.dv_count_batch_last_stats(C.byref(stats)) == _lib.DV_OK
  assert A.last_batch_stats()._fields == tuple(name for name, _ in _lib.DvCountBatchStats._fields_)   # pylint: disable=protected-access


def test_the_switch_is_off_by_default(monkeypatch):
  monkeypatch.delenv('DV_COUNT_ONE_LAUNCH', raising=False)
  assert not A.count_one_launch()
  monkeypatch.setenv('DV_COUNT_ONE_LAUNCH', '1')
  assert A.count_one_launch()


def test_batch_layout_with_the_one_launch_sections(tmp_path):
  """plan_batch with and without one_launch against the tool's own statement of every offset.  The tool of the
  commit before the switch printed `513216 cases, 0 mismatches`; with the one_launch cases it prints
  `653184 cases, 0 mismatches`, the earlier cases among them unchanged."""
  hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
  exe = str(tmp_path / 'count_batch_layout_check')
  subprocess.check_call([hipcc, '-std=c++17', '-O1', '-I' + os.path.join(ROOT, 'include'),
                         '-I' + os.path.join(ROOT, 'deepvariant_amd', 'csrc'),
                         os.path.join(ROOT, 'tools', 'count_batch_layout_check.cpp'), '-o', exe])
  out = subprocess.check_output([exe]).decode()
  assert re.search(r'^\d+ cases, 0 mismatches$', out.strip().splitlines()[-1])
  assert int(out.strip().splitlines()[-1].split()[0]) > 513216


@pytest.mark.parametrize('make', [L.block_edge_batch, L.special_batch])
def test_cases_hold_their_block_counts(make):
  case = make()
  tables = [packing.ReadTable.from_reads(list(rs)) if rs else None for rs in case.reads]
  n_reads = [len(t.read_pos) if t is not None else 0 for t in tables]
  want = [-(-n // 64) if n and e > s else 0 for n, (s, e) in zip(n_reads, case.spans)]
  assert list(case.blocks) == want and case.total_blocks == sum(want)
  slots = L.batched_regions(case)
  assert all(b >= 1 for b in (case.blocks[k] for k in slots))
  if case.name == 'block_edge':
    assert [n_reads[k] for k in slots] == list(L.EDGE_READ_COUNTS)
    assert [case.blocks[k] for k in slots] == [1, 1, 1, 2, 2, 2, 3, 4, 1, 1] and case.total_blocks == 18
    assert case.kinds[2] == 'readless' and n_reads[2] == 0
    s, e = case.spans[6]
    assert case.kinds[6] == 'zero_length' and s == e and n_reads[6] > 64     # reads, and still no slot
    assert slots != list(range(len(slots))) and slots[2] == 3 and slots[-1] == len(case.spans) - 1
    assert len({s % 1000 for s, _ in case.spans}) > 3                       # different contig offsets
    for k in slots:                                                          # 40 to 60 reference bases a read
      t = tables[k]
      assert np.all(np.diff(t.read_pos.astype(np.int64)) >= 0)
      span = t.read_end.astype(np.int64) - t.read_pos.astype(np.int64)
      assert span.min() >= 40 and span.max() <= 63
  else:
    assert case.kinds == ('neighbour', 'wide', 'events', 'legacy', 'neighbour') and slots == [0, 1, 2, 3, 4]
    assert list(case.blocks) == [1, 1, 1, 2, 2]
    wide = tables[1]
    pos, end = wide.read_pos.astype(np.int64), wide.read_end.astype(np.int64)
    assert n_reads[1] <= 64 and end.max() - pos[0] > L.WINDOW and pos.min() < pos[0]
    noisy = case.reads[2]
    mismatches = sum(sum(a != b for a, b in zip(r.aligned_sequence, case.ref.seq[r.alignment.position.position:]))
                     for r in noisy)
    assert len(noisy) == 64 and mismatches > L.BLOCK_EVENTS
    assert len(tables[2].cigar) + len(tables[2].bases) // 16 + 4096 > mismatches   # within the batch's first guess
    legacy, plain = case.options[3], case.options[0]
    assert legacy['keep_legacy_behavior'] and not plain['keep_legacy_behavior']
    assert legacy['min_mapping_quality'] > plain['min_mapping_quality']
    assert legacy['min_base_quality'] > plain['min_base_quality']
    assert len({r.alignment.mapping_quality >= legacy['min_mapping_quality'] for r in case.reads[3]}) == 2
  positions = L.candidate_positions(case)
  with_positions = [bool(positions[k]) for k in slots]
  assert with_positions == [i % 2 == 0 for i in range(len(slots))]           # a null mask beside a real one
  assert not any(positions[k] for k in range(len(case.spans)) if k not in slots)
