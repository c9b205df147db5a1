"""Shared test helpers: golden fixture access and mode names."""
import hashlib
import json
from functools import lru_cache
from pathlib import Path

import numpy as np

GOLDEN = Path(__file__).resolve().parent / "golden"

MODE_IDS = {"tensor_asym": 0, "tensor_sym": 1, "channel_asym": 2, "channel_sym": 3}


def h(a) -> str:
    """sha256 of fp32 bytes with -0 folded into +0 (as tests/golden/make_golden.py)."""
    a = np.ascontiguousarray(np.asarray(a, dtype=np.float32)) + np.float32(0.0)
    return hashlib.sha256(a.tobytes()).hexdigest()


def hb(a) -> bytes:
    return bytes.fromhex(h(a))


def quant_cases():
    z = np.load(GOLDEN / "quant_cases.npz", allow_pickle=False)
    meta = json.loads(str(z["meta"]))
    out = []
    for i, m in enumerate(meta):
        case = dict(m)
        case["idx"] = i
        case["x"] = z[f"in{m['input']}"]
        case["dq"] = z[f"dq{i}"] if f"dq{i}" in z.files else None
        case["dqh"] = str(z[f"dqh{i}"])
        case["esum_ref"] = z[f"esum{i}"] if f"esum{i}" in z.files else None
        out.append(case)
    return out


def case_flags(case):
    """(mode, rows, flags, given) for the oracle/kernels."""
    mode = MODE_IDS[case["mode"]]
    x = case["x"]
    rows = x.shape[0] if mode >= 2 else 1
    flags = 0
    given = (0.0, 0.0)
    if case["given"] is not None:
        flags |= 2
        given = tuple(case["given"])
    if case["default_range"]:
        flags |= 4
    if case["clip"] is not None:
        flags |= 1
    return mode, rows, flags, given


def transform_cases():
    z = np.load(GOLDEN / "transform_cases.npz", allow_pickle=False)
    return z, json.loads(str(z["meta"]))


@lru_cache(maxsize=1)
def bc_edge():
    """tests/golden/bc_edge_cases.npz cut by the case lists of tests/bc_edge_cases.py:
    {"apply": {name: {threads: bias_out}}, "prop": {name: {threads: fb_out}},
    "expect": {name: vector}, "digest": {name: hex}} (read-only arrays; a result
    that does not depend on the thread count is the same array under every count)."""
    from tests import bc_edge_cases as BE
    z = np.load(GOLDEN / "bc_edge_cases.npz", allow_pickle=False)

    def cut(flat, cases, width):
        out, at = {}, 0
        for c in cases:
            n = width(c)
            rows = flat[at:at + n * (len(BE.THREADS) if c.threaded else 1)].reshape(-1, n)
            at += rows.size
            out[c.name] = {t: rows[k if c.threaded else 0] for k, t in enumerate(BE.THREADS)}
        assert at == flat.size
        return out

    flat = {k: z[k] for k in ("apply_bias_out", "prop_fb_out", "expect")}
    for a in flat.values():
        a.setflags(write=False)
    ex = flat["expect"].reshape(len(BE.EXPECT_CASES), BE.EXPECT_N)
    names = [c.name for c in BE.APPLY_CASES] + [c.name for c in BE.PROP_CASES] + ["expect"]
    digests = [str(d) for d in z["digests"]]
    assert len(names) == len(digests)
    return {"apply": cut(flat["apply_bias_out"], BE.APPLY_CASES, lambda c: c.o),
            "prop": cut(flat["prop_fb_out"], BE.PROP_CASES, lambda c: c.F),
            "expect": {case[0]: ex[k] for k, case in enumerate(BE.EXPECT_CASES)},
            "digest": dict(zip(names, digests))}


@lru_cache(maxsize=1)
def act_edge():
    """tests/golden/act_edge_cases.npz by graph (tests/act_edge_cases.py GRAPHS):
    {graph: {"rec": [(kind, vector), ...] in the reference's call order, "min",
    "max" (every quantizer: target layers, then the tensor-op inputs), "targets",
    "op_keys", "digest"}} (read-only arrays)."""
    from tests import act_edge_cases as AE
    z = np.load(GOLDEN / "act_edge_cases.npz", allow_pickle=False)
    pool, ends = z["pool"], np.cumsum(z["pool_len"])
    pool.setflags(write=False)
    vec = [pool[e - n:e] for e, n in zip(ends, z["pool_len"])]
    out = {}
    for g in AE.GRAPHS:
        out[g] = {"rec": [(int(k), vec[i]) for k, i in zip(z[f"{g}.kinds"], z[f"{g}.seq"])],
                  "min": z[f"{g}.min"], "max": z[f"{g}.max"], "targets": list(z[f"{g}.targets"]),
                  "op_keys": [str(k) for k in z[f"{g}.op_keys"]], "digest": str(z[f"{g}.digest"])}
    return out


def pipeline(name, threads=8, bits_weight=8):
    """The reference's main_dfq stage order on the synthetic model, run with
    ``threads`` torch intra-op threads (tests/golden/make_golden.py:pipeline);
    ``bits_weight`` 4: the --bits_weight 4 run (pipeline_<name>_w4.npz, 8 threads)."""
    if bits_weight != 8:
        assert threads == 8, "the W4 fixtures are 8-thread runs"
        return np.load(GOLDEN / f"pipeline_{name}_w{bits_weight}.npz", allow_pickle=False)
    f = f"pipeline_{name}.npz" if threads == 8 else f"pipeline_{name}_t{threads}.npz"
    return np.load(GOLDEN / f, allow_pickle=False)


def recover_codes_consistent(dq, codes, scale, zero):
    """dq == fl(fl(code * s) + zero) elementwise (codes regenerate the output)."""
    s = np.float32(scale)
    z = np.float32(zero)
    regen = (codes.astype(np.float32) * s).astype(np.float32) + z
    return np.array_equal(regen.astype(np.float32), dq)


def chunk_cases():
    """quantize() with num_chunks / a None bound (tests/golden/chunk_cases.npz)."""
    z = np.load(GOLDEN / "chunk_cases.npz", allow_pickle=False)
    meta = json.loads(str(z["meta"]))
    out = []
    for i, m in enumerate(meta):
        case = dict(m)
        case["idx"] = i
        case["x"] = z[f"in{m['input']}"]
        if m["error"] is None:
            case["range"] = z[f"range{i}"]
            case["dq"] = z[f"dq{i}"]
            case["dqh"] = str(z[f"dqh{i}"])
        out.append(case)
    return out


def chunk_kwargs(case):
    """quantize() keyword arguments of a chunk case."""
    kw = dict(symmetric=case["sym"], num_chunks=case["num_chunks"])
    if case["given"] is not None:
        kw[f"{case['given'][0]}_value"] = case["given"][1]
    return kw
