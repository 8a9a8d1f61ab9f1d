"""bench.py's modes (CPU only, no GPU touched): a plain run is the headline
alone, --full adds every other measurement, --dump-outputs names a folder."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_defaults_are_a_plain_run():
    import bench
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (a.gpus, a.steps, a.warmup) == (1, 7, 2)
    assert a.full is False and a.dump_outputs is None


def test_full_and_dump_outputs_parse():
    import bench
    a = bench.parse(["--full", "--dump-outputs", "some/dir", "--no-config2"])
    assert a.full is True and a.dump_outputs == "some/dir" and a.no_config2 is True


def test_no_headline_needs_full(capsys):
    import torch
    import bench
    with pytest.raises(SystemExit) as e:  # refused before anything is set up
        bench.main(["--gpus", "1", "--no-headline"])
    assert e.value.code == 2
    assert "--full" in capsys.readouterr().err
    assert not torch.cuda.is_initialized()
