"""bench.py's plain run and --dump-outputs: the plain line carries the headline only, and the dump holds what the timed
path's last step computed, from inputs that are the same on every run (CPU: the --stub-cpu rank program; GPU: configs[1])."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

FULL_ONLY = ("value_spread", "roofline", "roofline_isolated", "roofline_kernels", "raw_c_abi_loop", "one_bag_in_flight",
             "module_call", "module_call_bf16", "amp_bf16", "f32x3", "h2d_inclusive", "rrtmil_c16", "train_step", "config0",
             "config2", "config3", "config4", "fresh_inputs", "cpu_baseline")


def _run_bench(*argv, timeout=300):
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "TORCHELASTIC_RUN_ID"):
        env.pop(k, None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *argv], capture_output=True, text=True,
                         timeout=timeout, env=env, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout
    return json.loads(lines[0])


def test_dump_outputs_stub_same_on_every_run(tmp_path):
    args = ("--stub-cpu", "--steps", "3", "--warmup", "1", "--config", "4", "--dump-outputs")
    a, b = _run_bench(*args, str(tmp_path / "a")), _run_bench(*args, str(tmp_path / "b"))
    assert a["steps"] == b["steps"] == 3
    assert os.listdir(tmp_path / "a") == os.listdir(tmp_path / "b") == ["bag_sums.npy"]
    x, y = np.load(tmp_path / "a" / "bag_sums.npy"), np.load(tmp_path / "b" / "bag_sums.npy")
    assert x.dtype == np.float64 and x.shape == (64,) and np.isfinite(x).all() and np.array_equal(x, y)
    # two ranks: each writes its own share of the 64 bags
    _run_bench("--gpus", "2", *args, str(tmp_path / "c"))
    parts = [np.load(tmp_path / "c" / f"bag_sums_rank{r}.npy") for r in range(2)]
    assert sorted(os.listdir(tmp_path / "c")) == ["bag_sums_rank0.npy", "bag_sums_rank1.npy"]
    assert sum(p.size for p in parts) == 64 and np.allclose(np.sort(np.concatenate(parts)), np.sort(x))


@pytest.mark.gpu
def test_plain_run_headline_and_dump_outputs(tmp_path, monkeypatch):
    """configs[1] as the plain command runs it: one line without any --full record, `steps` timed steps of 256 bags, and a
    dump whose rows are those of the module's own forward of the same bags."""
    import torch
    monkeypatch.setattr(os, "environ", dict(os.environ))     # bench.py sets HIP defaults at import: not for later tests
    import bench
    from rrt_mil_amd import RRTEncoder, synth
    rec = _run_bench("--gpus", "1", "--steps", "2", "--warmup", "1", "--dump-outputs", str(tmp_path), timeout=600)
    assert not set(FULL_ONLY) & set(rec), sorted(set(FULL_ONLY) & set(rec))
    assert rec["steps"] == 2 and rec["unit"] == "slides/s" and rec["higher_is_better"] is True and rec["dtype"] == "f32"
    nb = rec["config"]["bags_per_step"]
    assert abs(rec["value"] - nb / (rec["ms_per_step"] * 1e-3)) / rec["value"] < 1e-3
    assert os.listdir(tmp_path) == ["y.npy"]
    y = np.load(tmp_path / "y.npy")
    assert os.path.getsize(tmp_path / "y.npy") <= 64 << 20
    assert y.dtype == np.float32 and y.shape[0] == nb and y.shape[2] == 512 and np.isfinite(y).all()
    # bag j of the call is input bag j % 4 (bench.py: EncoderWorkload.call_bags)
    cfg = bench.CONFIGS[1]["enc"]
    enc = RRTEncoder(**cfg).eval()
    st = synth.encoder_state(**{k: v for k, v in cfg.items() if k != "region_num"})
    enc.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in st.items()}, strict=True)
    enc = enc.to("cuda:0")
    idx = bench.sample_index(9000, y.shape[1])
    for j in range(4):
        x = torch.from_numpy(synth.bag(9000, 512, tag=f"bench/r0/b{j}")).to("cuda:0")
        with torch.no_grad():
            ref = enc(x.unsqueeze(0)).squeeze(0)[torch.from_numpy(idx).to("cuda:0")].cpu().numpy()
        for b in (j, j + 4, nb - 4 + j):
            assert np.abs(y[b] - ref).max() < 1e-3, (j, b, float(np.abs(y[b] - ref).max()))
