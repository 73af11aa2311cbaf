"""bench.py's command line: a plain run measures the headline only, `--full` adds the rest."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
  sys.path.insert(0, ROOT)

import bench  # noqa: E402


def _parse(monkeypatch, *argv):
  monkeypatch.setattr(sys, 'argv', ['bench.py'] + list(argv))
  return bench.parse_args()


def test_plain_run_is_not_full(monkeypatch):
  args = _parse(monkeypatch, '--gpus', '1', '--steps', '20', '--warmup', '5')
  assert not args.full
  assert (args.gpus, args.steps, args.warmup) == (1, 20, 5)


def test_full_keeps_its_refinements(monkeypatch):
  args = _parse(monkeypatch, '--full', '--no-cpu-baseline', '--no-workloads', '--no-dense')
  assert args.full and args.no_cpu_baseline and args.no_workloads and args.no_dense


def test_dump_outputs_still_needs_resident_mode(monkeypatch):
  with pytest.raises(SystemExit):
    _parse(monkeypatch, '--mode', 'host', '--dump-outputs', 'd')
