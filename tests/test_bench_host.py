"""bench.py's argument checks, without a GPU."""
import pytest

import bench


def test_steps_and_dump_outputs_arguments():
    a = bench.parse(["--steps", "7", "--warmup", "2", "--dump-outputs", "out"])
    assert a.steps == 7 and a.warmup == 2 and a.dump_outputs == "out" and a.mode == "batch"
    assert bench.parse([]).dump_outputs is None
    with pytest.raises(SystemExit):
        bench.parse(["--steps", "0"])  # not quietly one step
    with pytest.raises(SystemExit):
        bench.parse(["--mode", "stream", "--dump-outputs", "out"])  # a stream step has no output batch to dump
