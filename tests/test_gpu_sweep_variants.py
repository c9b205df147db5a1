"""Every sweep kernel variant of the diagnostics library (kVariants, dfq_sweep_plan.h) against
the C oracle, bit for bit, on one small list (fresh process, DFQ_LIB=diag, DFQ_SWEEP_VARIANT).

pytest otherwise runs variants 6, 10 and 16 only; the prefetch loop (1, 2, 11), the IEEE divide on
every element (14), the generic float4 loop (15), the timeline variant with no buffer set (13) and
the KH*KW sum forms (ESPEC 0 and 2) are reached from scripts/ alone.  The list holds the smallest
shapes that reach each task kind at every chunk size (1,024 .. 4,096):

  (64, 32, 3, 3)   several 288-element rows per task, KH*KW = 9; on variant 16 the two-batch split
  (3, 512, 3, 3)   4,608-element rows: block-row pieces at 2,048 / 4,096, slot pieces at 1,024
  (2, 160, 7, 7), (4, 8, 5, 5), (8, 16, 2, 2), (6, 10, 1, 3)   KH*KW 49, 25, 4 and 3 (generic sum)
  (2, 8192), (2, 8193), (3, 2051), (5, 1025, 1, 1)   block-row and slot pieces, vec4 and scalar
  (33, 13), (7, 27), (1, 1), (0, 9)   the scalar path, one element, an empty tensor
  (2, 20000)       slot pieces

each in all four modes (clip on in mode 3), at 8, 5, 4 (packed nibbles where the planner takes the
shape at that variant's chunk, plain codes where it does not) and 12 bits (int16 codes), with and
without the error sums.  dst, codes, scale, zero (after + float32(0)) and esum of every item are
compared with oracle.quantize; an empty tensor has no range, so in the per-tensor modes nothing is
written to its scale / zero and they are not compared.  Outputs live in one arena that is
overwritten before every variant, so a variant that wrote nothing cannot pass on the last one's bytes.
"""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_SCRIPT = r"""
import json, math, os, sys
sys.path.insert(0, os.environ["DFQ_ROOT"])
import numpy as np
import torch
from data_free_quantization_amd.sweep import SweepItem, SweepPlan, allocate, code_dtype
from oracle import oracle as O
dev = torch.device("cuda:0")
SHAPES = [(64, 32, 3, 3), (3, 512, 3, 3), (2, 160, 7, 7), (4, 8, 5, 5), (8, 16, 2, 2), (6, 10, 1, 3),
          (2, 8192), (2, 8193), (3, 2051), (5, 1025, 1, 1), (33, 13), (7, 27), (1, 1), (0, 9), (2, 20000)]
CLIP = (-1.0, 1.0)
FIELDS = ("dst", "codes", "scale", "zero", "esum")

# the cases and their oracle results, once for all variants
cases = []
for si, shp in enumerate(SHAPES):
    x = np.random.default_rng(100 + si).normal(0, 1, shp).astype(np.float32)
    xd = torch.from_numpy(x).to(dev)
    khw = math.prod(shp[2:]) if len(shp) >= 3 else 1
    for mode in range(4):
        for bits in (8, 5, 4, 12):
            for esum in (True, False):
                o = O.quantize(x, bits, mode, rows=shp[0] if mode >= 2 else 1, khw=khw, flags=O.F_CLIP if mode == 3 else 0,
                               clip=CLIP, want_esum=esum)
                cases.append(dict(shape=shp, x=x, xd=xd, khw=khw, mode=mode, bits=bits, esum=esum, o=o))


def pack_nibbles(codes):
    c = codes.reshape(-1).astype(np.uint8) & 0xF
    c = np.append(c, np.zeros(c.size % 2, np.uint8))
    return c[0::2] | (c[1::2] << 4)


def packs(c):
    # packed nibbles where the library takes the shape at this variant's chunk
    if c["bits"] != 4:
        return False
    try:
        SweepPlan([allocate(c["xd"], bits=4, per_channel=c["mode"] >= 2, symmetric=c["mode"] in (1, 3), khw=c["khw"],
                            pack_int4=True)]).destroy()
        return True
    except (NotImplementedError, ValueError):
        return False


def run_variant(v):
    os.environ["DFQ_SWEEP_VARIANT"] = str(v)
    # every output in one arena (256-B aligned pieces): one fill before, one copy back after
    spans, off = [], 0
    for c in cases:
        n, sym, ch = c["x"].size, c["mode"] in (1, 3), c["mode"] >= 2
        c["pack"] = packs(c)
        npar = c["shape"][0] if ch else 1
        cdt = torch.uint8 if c["pack"] else code_dtype(c["bits"], sym)
        want = {"dst": (torch.float32, n), "codes": (cdt, (n + 1) // 2 if c["pack"] else n), "scale": (torch.float32, npar),
                "zero": (torch.float32, npar), "esum": (torch.float32, n // c["khw"]) if c["esum"] else None}
        sp = {}
        for f in FIELDS:
            if want[f] is not None:
                nb = want[f][1] * torch.empty(0, dtype=want[f][0]).element_size()
                sp[f] = (off, nb, want[f][0])
                off += (nb + 255) // 256 * 256
        spans.append(sp)
    arena = torch.full((max(off, 256),), 0xA5, dtype=torch.uint8, device=dev)
    items = []
    for c, sp in zip(cases, spans):
        t = {f: arena[o:o + nb].view(dt) for f, (o, nb, dt) in sp.items()}
        items.append(SweepItem(src=c["xd"], bits=c["bits"], per_channel=c["mode"] >= 2, symmetric=c["mode"] in (1, 3),
                               dst=t["dst"].view(c["shape"]), codes=t["codes"], scale=t["scale"], zero=t["zero"],
                               esum=t.get("esum"), khw=c["khw"], clip=CLIP if c["mode"] == 3 else None,
                               rows=c["shape"][0] if c["mode"] >= 2 else 1, pack_int4=c["pack"]))
    plan = SweepPlan(items)
    got_v = plan.stats["variant"]
    plan.execute()
    torch.cuda.synchronize()
    host = arena.cpu().numpy()
    plan.destroy()
    bad = []
    for c, sp in zip(cases, spans):
        o = c["o"]
        np_of = lambda f: host[sp[f][0]:sp[f][0] + sp[f][1]]   # noqa: E731
        ne = {"dst": not np.array_equal(np_of("dst").view(np.float32), o["dq"].reshape(-1))}
        if c["pack"]:
            ne["codes"] = not np.array_equal(np_of("codes"), pack_nibbles(o["codes"]))
        else:
            ne["codes"] = not np.array_equal(np_of("codes").view(o["codes"].dtype), o["codes"].reshape(-1))
        if c["x"].size or c["mode"] >= 2:   # an empty tensor has no per-tensor range: nothing is written
            ne["scale"] = not np.array_equal(np_of("scale").view(np.float32), o["scale"])
            ne["zero"] = not np.array_equal(np_of("zero").view(np.float32) + np.float32(0), o["zero"] + np.float32(0))
        if c["esum"]:
            ne["esum"] = not np.array_equal(np_of("esum").view(np.float32), o["esum"])
        if any(ne.values()):
            bad.append([list(c["shape"]), c["mode"], c["bits"], c["esum"], c["pack"], sorted(f for f in ne if ne[f])])
    return {"variant": v, "plan_variant": got_v, "items": len(items), "packed": sum(c["pack"] for c in cases),
            "mismatched": len(bad), "first": bad[:8]}


# kNumVariants: the first forced number the planner does not take (it then plans the default)
tiny = allocate(torch.zeros(4, 8, device=dev))
nvar = 0
while True:
    os.environ["DFQ_SWEEP_VARIANT"] = str(nvar)
    p = SweepPlan([tiny])
    ok = p.stats["variant"] == nvar
    p.destroy()
    if not ok:
        break
    nvar += 1
print("RESULT " + json.dumps({"variants": nvar, "runs": [run_variant(v) for v in range(nvar)]}))
"""


def test_every_variant_matches_oracle():
    env = dict(os.environ, DFQ_ROOT=ROOT, DFQ_LIB="diag", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", _SCRIPT], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    print(json.dumps(res))
    assert res["variants"] >= 17, res["variants"]   # the table's rows today (0..16); none may be lost
    assert [x["variant"] for x in res["runs"]] == list(range(res["variants"]))
    for x in res["runs"]:
        assert x["plan_variant"] == x["variant"], x
        assert x["items"] == 15 * 4 * 4 * 2 and x["packed"] > 0, x
        assert x["mismatched"] == 0, x
