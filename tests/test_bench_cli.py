"""bench.py's command line: a plain run measures the headline figure and nothing else; every other leg waits behind --full.
bench.py runs in a child process (it sets process-wide runtime defaults before its first HIP call)."""
import json
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(REPO, "bench.py")
CONTRACT = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("roofline", "cpu_baseline", "val_dice", "max_rel_logit_err", "host_enqueue_ms_per_step")


def test_full_is_an_option_and_off_by_default():
    r = subprocess.run([sys.executable, BENCH, "--help"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "--full" in r.stdout and "--dump-outputs" in r.stdout
    r = subprocess.run([sys.executable, BENCH, "--full=1"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "--full" in r.stderr            # a switch, not a valued option: off unless given


@pytest.mark.gpu
def test_plain_run_prints_the_headline_line_and_skips_every_other_leg(tmp_path):
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "2", "--warmup", "1", "--dump-outputs", str(tmp_path / "out")],
                       capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    for k in CONTRACT:
        assert k in out, k
    assert out["full"] is False and out["steps"] == 2 and out["warmup"] == 1 and out["higher_is_better"] is True
    assert out["unit"] == "volumes/s" and out["value"] > 0 and out["ms_per_step"] > 0
    assert abs(out["value"] - 2 * 1000.0 / out["ms_per_step"]) <= 0.01 * out["value"]      # batch 2 per step: the same quantity twice
    for k in FULL_ONLY:
        assert k not in out, k
    for leg in ("cpu_baseline", "roofline leg", "val_dice leg"):
        assert leg not in r.stderr, leg
    assert os.path.exists(tmp_path / "out" / "loss.npy") and os.path.exists(tmp_path / "out" / "loss_parts.npy")
