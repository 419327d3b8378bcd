"""bench.py's own contract: a plain run times the headline and nothing else, --full keeps every other leg, --dump-outputs writes the last
timed step's results reproducibly (so that two builds can be compared output for output)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--steps", "3", "--warmup", "1", "--width", "640", "--height", "400", "--layers", "6", "--sigma", "3.0"]


def _bench(extra):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + SMALL + extra, capture_output=True, text=True, cwd=ROOT, timeout=600)
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert p.returncode == 0 and len(lines) == 1, p.stdout[-2000:] + p.stderr[-2000:]
    return json.loads(lines[0])


def test_dump_outputs_writes_a_fixed_float32_sample_within_64_mb(tmp_path):
    import torch
    sys.path.insert(0, ROOT)
    import bench
    g = torch.Generator().manual_seed(11)
    frame = torch.randint(0, 256, (bench.H8K, bench.W8K, 4), dtype=torch.uint8, generator=g)
    small = frame[:300, :500].contiguous()
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"flatten": frame, "gaussian": frame, "small": small})
    total = 0
    for name in ("flatten", "gaussian", "small"):
        a, b = np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")
        assert a.dtype == np.float32 and np.array_equal(a, b)
        total += os.path.getsize(tmp_path / "a" / f"{name}.npy")
    assert total - os.path.getsize(tmp_path / "a" / "small.npy") <= 64 << 20   # the headline's two 8K outputs
    idx = np.sort(np.random.default_rng(bench.DUMP_SEED).choice(bench.H8K * bench.W8K, size=bench.DUMP_MAX_PX, replace=False))
    assert np.array_equal(np.load(tmp_path / "a" / "flatten.npy"), frame.reshape(-1, 4).numpy()[idx].astype(np.float32))
    assert np.array_equal(np.load(tmp_path / "a" / "small.npy"), small.numpy().astype(np.float32))   # small frames whole, (h, w, 4)


def test_dump_outputs_is_refused_outside_the_single_gpu_headline():
    for extra in (["--gpus", "2"], ["--config", "batch4k"]):
        p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--dump-outputs", "unused"] + extra, capture_output=True, text=True, cwd=ROOT,
                           timeout=120)
        assert p.returncode == 2 and "--dump-outputs" in p.stderr


@pytest.mark.gpu
def test_plain_run_is_the_headline_alone_and_dumps_what_it_computed(tmp_path):
    import torch
    sys.path.insert(0, ROOT)
    import bench
    from tests import oracle_lib as O
    d = _bench(["--dump-outputs", str(tmp_path / "a")])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["unit"] == "Mpixels/s" and d["higher_is_better"] is True and d["value"] > 0
    assert abs(d["value"] - 640 * 400 / d["ms_per_step"] / 1e3) / d["value"] < 0.01
    assert d["dtype"].startswith("f32") and d["metric"].startswith("Mpixels/sec")
    for k in ("check", "cpu_baseline", "c_abi_group", "configs", "value_exact_f32", "exact_f32_leg"):
        assert k not in d, k
    assert "traffic_live" not in d["roofline"] and "clock_power" not in d["roofline"]
    # the same arguments give the same inputs, hence the same outputs
    _bench(["--dump-outputs", str(tmp_path / "b")])
    for name in ("flatten", "gaussian"):
        assert np.array_equal(np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")), name
    # and they are the timed pipeline's results: the oracle on bench.py's own stack (rank 0's seed)
    stack, modes, opac = bench.synth_stack(torch, torch.device("cuda", 0), 640, 400, 6, seed=0x5EED0002)
    ref = O.flatten_stack(stack.cpu().numpy(), modes, opac)
    flat = np.load(tmp_path / "a" / "flatten.npy")
    assert flat.dtype == np.float32 and flat.shape == (400, 640, 4) and np.array_equal(flat, ref.astype(np.float32))
    blur = np.load(tmp_path / "a" / "gaussian.npy")
    assert np.abs(blur - O.gaussian_blur(ref, 3.0).astype(np.float32)).max() <= 1   # matrix-core Gaussian: the stated +-1 LSB


@pytest.mark.gpu
def test_full_run_keeps_the_other_legs():
    d = _bench(["--full", "--no-live-pmc"])
    assert d["value"] > 0 and "failed_checks" not in d
    assert d["check"]["flatten_crop_bitexact"] is True and d["check"]["flatten_whole_frame_bitexact"] is True
    assert d["cpu_baseline"]["value"] > 0 and d["value_exact_f32"] > 0 and d["exact_f32_leg"]["gaussian_whole_frame_bitexact"] is True
    assert d["c_abi_group"]["check"]["identical_to_headline_result"] is True
