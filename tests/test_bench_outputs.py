"""bench.py's plain run and ``--dump-outputs``: a plain run carries the headline
keys and none of the ``--full`` legs, and the dump holds the timed path's outputs
as float32 arrays -- whole where a field is short, the same seeded sample of a long
field every time.  CPU: ``dump_outputs`` on host tensors.  GPU: the real bench on
one MobileNetV2 weight set."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

FULL_ONLY = ("parity", "memory_pattern_probe", "cpu_baseline", "secondary_configs", "single_model_latency",
             "pipeline_ms", "cle_roofline", "sharded_gathers", "weak_scaling", "configs4_sharded")


def _layers(seed):
    """Three layers: dq / codes longer than the sample cap in all, scale / zero short,
    no esum on the middle layer."""
    import bench
    g = torch.Generator().manual_seed(seed)
    sizes = [(bench.DUMP_MAX_ELEMS // 2 + 3, 7), (1025, 5), (bench.DUMP_MAX_ELEMS // 2 + 11, 9)]
    out = []
    for j, (n, rows) in enumerate(sizes):
        dq = torch.randn(n, generator=g)
        codes = torch.randint(-127, 128, (n,), generator=g, dtype=torch.int8)
        esum = None if j == 1 else torch.randn(n // 3, generator=g)
        out.append((dq, codes, torch.rand(rows, generator=g), torch.zeros(rows), esum))
    return out


def test_dump_outputs_whole_and_sampled(tmp_path):
    import bench
    layers = _layers(0)
    bench.dump_outputs(tmp_path / "a", layers, torch.device("cpu"))
    got = {f: np.load(tmp_path / "a" / f"{f}.npy") for f in bench.DUMP_FIELDS}
    assert all(a.dtype == np.float32 and a.ndim == 1 for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 64 << 20
    # short fields whole, in list order
    for f, name in ((2, "scale"), (3, "zero")):
        assert np.array_equal(got[name], torch.cat([lay[f] for lay in layers]).numpy())
    assert np.array_equal(got["esum"], torch.cat([layers[0][4], layers[2][4]]).numpy())
    # long fields: the sorted distinct positions drawn from a generator seeded with the length
    for f, name in ((0, "dq"), (1, "codes")):
        flat = torch.cat([lay[f].reshape(-1) for lay in layers]).to(torch.float32).numpy()
        assert flat.size > bench.DUMP_MAX_ELEMS
        pos = np.unique(np.random.default_rng(flat.size).integers(0, flat.size, bench.DUMP_MAX_ELEMS))
        assert pos[0] < layers[0][f].numel() < pos[-1]            # the sample spans the layers
        assert np.array_equal(got[name], flat[pos])
    # the same call again writes the same bytes; other values at the same positions differ
    bench.dump_outputs(tmp_path / "b", layers, torch.device("cpu"))
    bench.dump_outputs(tmp_path / "c", _layers(1), torch.device("cpu"))
    for f in bench.DUMP_FIELDS:
        assert (tmp_path / "b" / f"{f}.npy").read_bytes() == (tmp_path / "a" / f"{f}.npy").read_bytes()
    assert np.load(tmp_path / "c" / "dq.npy").shape == got["dq"].shape
    assert not np.array_equal(np.load(tmp_path / "c" / "dq.npy"), got["dq"])


def test_full_and_dump_options_default_off():
    import bench
    plain = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert not plain.full and plain.dump_outputs is None and plain.steps == 7 and plain.warmup == 2
    assert bench.parse(["--full"]).full
    assert bench.parse(["--dump-outputs", "d"]).dump_outputs == "d"


@pytest.mark.gpu
def test_bench_plain_run_dumps_its_outputs(tmp_path):
    """One MobileNetV2 weight set, 4 timed steps: the line holds the headline keys
    with ``steps`` as asked and every ``--full`` leg null; the dump is the sampled
    dq / codes (same positions: dq is codes x the row's scale, so |dq| <= 127 x the
    largest scale and a zero code is a zero dq) and whole scale / zero."""
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "1",
                        "--copies", "1", "--prewarm-ms", "0", "--dump-outputs", str(tmp_path / "out")],
                       capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    res = lines[0]
    assert res["steps"] == 4 and len(res["timing"]["step_ms"]) == 4 and res["ms_per_step"] > 0
    assert res["unit"] == "GB/s" and res["higher_is_better"] is True and res["dtype"] == "f32" and res["value"] > 0
    assert all(res[k] is None for k in FULL_ONLY), [k for k in FULL_ONLY if res[k] is not None]
    assert res["timing"]["telemetry"] is None
    import bench
    got = {f: np.load(tmp_path / "out" / f"{f}.npy") for f in bench.DUMP_FIELDS}
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 64 << 20
    n = res["config"]["weights_per_copy"]
    assert n > bench.DUMP_MAX_ELEMS
    want = np.unique(np.random.default_rng(n).integers(0, n, bench.DUMP_MAX_ELEMS)).size
    assert got["dq"].size == got["codes"].size == want
    assert got["scale"].size == got["zero"].size and (got["scale"] > 0).all()
    assert np.abs(got["codes"]).max() == 127 and np.array_equal(got["codes"], np.round(got["codes"]))
    assert np.abs(got["dq"]).max() <= 127 * got["scale"].max()
    assert np.array_equal(got["dq"] == 0, got["codes"] == 0)
