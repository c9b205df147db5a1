"""High-bias absorption (dfq_bias_absorb, dfq_bias_absorb_batch: csrc/dfq_transform.hip)
on relations at the edges of its kernels: channel counts around the wave's 64
lanes, output rows that are no multiple of a GEMV task's 4 rows, dense /
depthwise / 2-group / Linear second layers, 1 / 9 / 25 taps.

Per relation, through both entry points:
  * b1 and the BN's fake_bias equal the CPU oracle bit for bit (elementwise fp32);
  * b2 of the batch call equals b2 of the per-relation call bit for bit
    (bias_absorption.py's docstring promises the same per-element order);
  * b2 is within a derived bound of a float64 reference.  With c in fp32 as every
    implementation has it and r = b2_in + sum_i sum_k w2[o,i,k] * c_i exactly
    (math.fsum of exact double products):
        |b2 - r| <= (khw2 + i2 + 2) * 2^-24 * sum_i sum_k |w2[o,i,k]| * c_i + 2^-24 * |b2|
    Any order of fp32 accumulation meets it: a tap sum of khw2 terms carries at
    most (khw2 - 1) roundings, its product with c_i one, the accumulation over
    i2 channels at most i2 (each relative 2^-24, first order, on partial sums
    bounded by the sum of magnitudes), and the final add to b2_in one more on
    the result.  A dropped lane or a wrong group index misses it by orders of
    magnitude.

Lists: a chain of relations that share bias vectors (in order and reversed)
equals the per-relation calls made in that order; a BN shared by two relations
and b1 == b2 are refused with nothing written; the shape the reference's matmul
rejects (c1 // (c1 // i2) != i2) is refused by both entry points.
"""
import ctypes as C
import math
from collections import OrderedDict

import numpy as np
import pytest
import torch
import torch.nn as nn

from data_free_quantization_amd import _lib
from oracle import oracle as O
from tests.bc_edge_cases import values

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
N_SIGMA = 3.0
C1S, KHWS, O2S = (1, 3, 63, 64, 65, 129, 257), (1, 9, 25), (1, 3, 5, 130)
KINDS = ("dense", "depthwise", "grouped2", "linear")


def _relation(seed, c1, kind, khw2, o2):
    """Host arrays of one relation: w2 [o2, i2, khw2] (2-D for Linear), b1, b2, the BN's
    fake_weight (gamma > 0) and fake_bias (beta = 3 * gamma + a value of either sign,
    so about half of c = max(beta - 3 * gamma, 0) clamps to 0)."""
    if kind == "depthwise":
        i2, o2 = 1, c1
    elif kind == "grouped2":
        i2, o2 = c1 // 2, 2 * o2      # o2 rows per group
    else:
        i2 = c1
    if kind == "linear":
        khw2 = 1
    w2 = values(seed, o2 * i2 * khw2, -26, -22).reshape((o2, i2) if kind == "linear" else (o2, i2, khw2))
    gamma = np.abs(values(seed + 1, c1, -27, -24)) + np.float32(0.0625)
    beta = np.float32(N_SIGMA) * gamma + values(seed + 2, c1, -26, -22)
    assert gamma.dtype == beta.dtype == np.float32
    return dict(w2=w2, b1=values(seed + 3, c1, -26, -22), b2=values(seed + 4, o2, -26, -22), bn_w=gamma, bn_b=beta,
                c1=c1, o2=o2, i2=i2, khw2=khw2)


def _cases():
    out, k = [], 0
    for kind in KINDS:
        for c1 in C1S:
            if kind == "grouped2" and c1 < 4:
                continue   # two groups need two channels each (c1 = 3, i2 = 1 is depthwise)
            khw2, o2 = KHWS[k % 3], O2S[(k // 2) % 4]
            out.append(pytest.param(7000 + 10 * k, c1, kind, khw2, o2, id=f"{kind}-c{c1}-k{khw2}-o{o2}"))
            k += 1
    # every tap count and every row count meets a dense and a grouped second layer
    for j, (khw2, o2) in enumerate([(k2, o) for k2 in KHWS for o in O2S]):
        out.append(pytest.param(8000 + 10 * j, 65, "dense" if j % 2 else "grouped2", khw2, o2,
                                id=f"sweep-{'dense' if j % 2 else 'grouped2'}-c65-k{khw2}-o{o2}"))
    return out


class _Dev:
    """A relation's vectors on the device (fresh copies of the host arrays)."""

    def __init__(self, r, shared=None):
        shared = shared or {}
        for k in ("w2", "b1", "b2", "bn_w", "bn_b"):
            setattr(self, k, shared[k] if k in shared else torch.from_numpy(r[k]).to(DEV).contiguous())
        self.r = r

    def desc(self):
        r = self.r
        return (self.w2.data_ptr(), self.b1.data_ptr(), self.b2.data_ptr(), self.bn_w.data_ptr(),
                self.bn_b.data_ptr(), r["c1"], r["o2"], r["i2"], r["khw2"])

    def out(self):
        torch.cuda.synchronize()
        return {k: getattr(self, k).cpu().numpy() for k in ("b1", "b2", "bn_w", "bn_b")}


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _single(d):
    w2, b1, b2, bw, bb, c1, o2, i2, khw2 = d.desc()
    return _lib.load().dfq_bias_absorb(w2, b1, b2, bw, bb, c1, o2, i2, khw2, N_SIGMA, _stream())


def _batch(devs):
    """(rc, failed relation) of one dfq_bias_absorb_batch call over devs."""
    L = _lib.load()
    descs = (_lib.AbsorbDesc * len(devs))()
    for x, d in zip(descs, devs):
        x.w2, x.b1, x.b2, x.bn_w, x.bn_b, x.c1, x.o2, x.i2, x.khw2 = d.desc()
    nb = int(L.dfq_bias_absorb_ws_bytes(descs, len(devs)))
    ws = torch.empty(max(nb, 256), dtype=torch.uint8, device=DEV)
    failed = C.c_int32(-1)
    rc = L.dfq_bias_absorb_batch(descs, len(devs), N_SIGMA, ws.data_ptr(), ws.numel(), C.byref(failed), _stream())
    torch.cuda.synchronize()
    return rc, failed.value, nb


def _bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))


def _b2_reference_and_bound(r):
    """(exact b2, bound) per output row; c in fp32 as the oracle computes it."""
    c = r["bn_b"] - np.float32(N_SIGMA) * r["bn_w"]
    assert c.dtype == np.float32
    c[c < 0] = 0
    o2, i2, khw2 = r["o2"], r["i2"], r["khw2"]
    w = r["w2"].reshape(o2, i2, khw2).astype(np.float64)
    o2g = o2 // (r["c1"] // i2)
    ref, bound = np.empty(o2), np.empty(o2)
    for o in range(o2):
        g = o // o2g
        prod = w[o] * c[g * i2:(g + 1) * i2].astype(np.float64)[:, None]   # exact: 24 x 24 bits
        ref[o] = math.fsum([float(r["b2"][o])] + prod.ravel().tolist())
        bound[o] = (khw2 + i2 + 2) * 2.0 ** -24 * math.fsum(np.abs(prod).ravel().tolist())
    return ref, bound, c


@pytest.mark.parametrize("seed,c1,kind,khw2,o2", _cases())
def test_relation_equals_oracle_and_float64_reference(seed, c1, kind, khw2, o2):
    r = _relation(seed, c1, kind, khw2, o2)
    ob1, ob2, _, ofb = O.bias_absorb(r["w2"], r["b1"], r["b2"], r["bn_w"], r["bn_b"], r["c1"], N_SIGMA)
    ref, bound, c = _b2_reference_and_bound(r)
    if c1 >= 63:
        assert 0.25 < (c == 0).mean() < 0.75, "about half of c clamps"
    one, bat = _Dev(r), _Dev(r)
    _lib.check(_single(one), "dfq_bias_absorb")
    rc, failed, _ = _batch([bat])
    _lib.check(rc, f"dfq_bias_absorb_batch (relation {failed})")
    got1, gotb = one.out(), bat.out()
    for tag, got in (("per-relation", got1), ("batch", gotb)):
        assert _bits(got["b1"], ob1), tag
        assert _bits(got["bn_b"], ofb), tag
        assert _bits(got["bn_w"], r["bn_w"]), tag
        err = np.abs(got["b2"].astype(np.float64) - ref)
        lim = bound + 2.0 ** -24 * np.abs(got["b2"].astype(np.float64))
        assert (err <= lim).all(), (tag, int(np.argmax(err - lim)), float((err / np.maximum(lim, 1e-300)).max()))
    assert _bits(got1["b2"], gotb["b2"]), "batch b2 != per-relation b2"
    # the oracle's own b2 meets the same bound (a sequential fp32 order)
    assert (np.abs(ob2.astype(np.float64) - ref) <= bound + 2.0 ** -24 * np.abs(ob2.astype(np.float64))).all()


# ---- lists ------------------------------------------------------------------
def _chain_hosts():
    """conv A(65) -> B(130) -> C(63) -> D(5): B's bias is b2 of relation 0 and b1 of
    relation 1, C's likewise for relations 1 and 2."""
    r0 = _relation(9100, 65, "dense", 9, 130)
    r1 = _relation(9200, 130, "dense", 1, 63)
    r2 = _relation(9300, 63, "dense", 25, 5)
    r1["b1"], r2["b1"] = r0["b2"], r1["b2"]
    return [r0, r1, r2]


def _chain_devs(hosts):
    d0 = _Dev(hosts[0])
    d1 = _Dev(hosts[1], shared={"b1": d0.b2})
    d2 = _Dev(hosts[2], shared={"b1": d1.b2})
    return [d0, d1, d2]


@pytest.mark.parametrize("order", [(0, 1, 2), (2, 1, 0)], ids=["in_order", "reversed"])
def test_list_sharing_biases_applies_in_relation_order(order):
    hosts = _chain_hosts()
    seq, bat = _chain_devs(hosts), _chain_devs(hosts)
    for k in order:
        _lib.check(_single(seq[k]), "dfq_bias_absorb")
    rc, failed, _ = _batch([bat[k] for k in order])
    _lib.check(rc, f"dfq_bias_absorb_batch (relation {failed})")
    for k in range(3):
        a, b = seq[k].out(), bat[k].out()
        for v in ("b1", "b2", "bn_b", "bn_w"):
            assert _bits(a[v], b[v]), (k, v)
        # each BN belongs to one relation: its result does not depend on the list
        alone = O.bias_absorb(hosts[k]["w2"], hosts[k]["b1"], hosts[k]["b2"], hosts[k]["bn_w"], hosts[k]["bn_b"],
                              hosts[k]["c1"], N_SIGMA)
        assert _bits(b["bn_b"], alone[3]), k
    # A's bias takes relation 0's update only: the oracle's b1
    assert _bits(bat[0].out()["b1"], O.bias_absorb(hosts[0]["w2"], hosts[0]["b1"], hosts[0]["b2"], hosts[0]["bn_w"],
                                                   hosts[0]["bn_b"], 65, N_SIGMA)[0])
    # the shared vectors really are order-dependent in fp32 for these inputs, so the two orders test something
    if order == (2, 1, 0):
        fwd = _chain_devs(hosts)
        for k in (0, 1, 2):
            _lib.check(_single(fwd[k]), "dfq_bias_absorb")
        assert not _bits(fwd[1].out()["b1"], bat[1].out()["b1"]) or not _bits(fwd[2].out()["b1"], bat[2].out()["b1"])


def _unchanged(devs, hosts):
    for d, r in zip(devs, hosts):
        got = d.out()
        for v in ("b1", "b2", "bn_w", "bn_b"):
            if not _bits(got[v], r[v]):
                return False
    return True


def test_shared_bn_is_unsupported_and_python_falls_back():
    ra = _relation(9400, 64, "dense", 9, 5)
    rb = _relation(9500, 64, "grouped2", 1, 3)
    rb["b1"], rb["bn_w"], rb["bn_b"] = ra["b1"], ra["bn_w"], ra["bn_b"]   # the same first layer and BN
    da = _Dev(ra)
    db = _Dev(rb, shared={"b1": da.b1, "bn_w": da.bn_w, "bn_b": da.bn_b})
    rc, failed, nb = _batch([da, db])
    assert (rc, failed, nb) == (_lib.DFQ_ERR_UNSUPPORTED, 1, -1)
    assert _unchanged([da, db], [ra, rb])
    # expected: the per-relation calls, in order
    for d in (da, db):
        _lib.check(_single(d), "dfq_bias_absorb")
    want_a, want_b = da.out(), db.out()
    # the Python entry point on a graph with one BN feeding two second layers
    from data_free_quantization_amd.bias_absorption import bias_absorption
    from data_free_quantization_amd.utils.relation import Relation
    conv1 = nn.Conv2d(8, 64, 1, bias=True)
    conv2 = nn.Conv2d(64, 5, 3, padding=1, bias=True)
    conv3 = nn.Conv2d(64, 6, 1, groups=2, bias=True)
    bn = nn.BatchNorm2d(64)
    with torch.no_grad():
        conv1.bias.copy_(torch.from_numpy(ra["b1"]))
        conv2.weight.copy_(torch.from_numpy(ra["w2"]).view(5, 64, 3, 3)); conv2.bias.copy_(torch.from_numpy(ra["b2"]))
        conv3.weight.copy_(torch.from_numpy(rb["w2"]).view(6, 32, 1, 1)); conv3.bias.copy_(torch.from_numpy(rb["b2"]))
    bn.register_buffer("fake_weight", torch.from_numpy(ra["bn_w"]).clone())
    bn.register_buffer("fake_bias", torch.from_numpy(ra["bn_b"]).clone())
    for m in (conv1, conv2, conv3, bn):
        m.to(DEV)
    graph = OrderedDict([("Data", "Data"), (1, conv1), (2, bn), (3, nn.ReLU()), (4, conv2), (5, conv3)])
    bottoms = OrderedDict([("Data", None), (1, ["Data"]), (2, [1]), (3, [2]), (4, [3]), (5, [3])])
    bias_absorption(graph, [Relation(1, 4, 2), Relation(1, 5, 2)], bottoms, N=3)
    torch.cuda.synchronize()
    assert _bits(conv1.bias.detach().cpu().numpy(), want_b["b1"])
    assert _bits(bn.fake_bias.cpu().numpy(), want_b["bn_b"])
    assert _bits(conv2.bias.detach().cpu().numpy(), want_a["b2"])
    assert _bits(conv3.bias.detach().cpu().numpy(), want_b["b2"])


def test_b1_equal_b2_is_a_shape_error():
    r = _relation(9600, 65, "dense", 1, 65)
    ok = _relation(9700, 3, "dense", 9, 5)
    d_ok = _Dev(ok)
    d = _Dev(r)
    d.b2 = d.b1
    r = dict(r, b2=r["b1"])
    rc, failed, nb = _batch([d_ok, d])
    assert (rc, failed, nb) == (_lib.DFQ_ERR_SHAPE, 1, -1)
    assert _unchanged([d_ok, d], [ok, r])


def test_channel_count_the_reference_rejects_is_a_shape_error():
    """c[start_inner:end_inner] has c1 // groups elements (bias_absorption.py:44,66), so
    the reference's matmul raises when c1 // (c1 // i2) != i2: c1 = 10, i2 = 4.  c1 = 9,
    i2 = 4 (groups 2, 4 channels each, the ninth in no group) it accepts."""
    bad = _relation(9800, 10, "dense", 9, 6)
    bad["i2"] = 4
    bad["w2"] = values(9801, 6 * 4 * 9, -26, -22).reshape(6, 4, 9)
    ok = _relation(9900, 3, "dense", 1, 5)
    for entry in ("per-relation", "batch"):
        d, d_ok = _Dev(bad), _Dev(ok)
        if entry == "per-relation":
            assert _single(d) == _lib.DFQ_ERR_SHAPE
        else:
            rc, failed, nb = _batch([d_ok, d])
            assert (rc, failed, nb) == (_lib.DFQ_ERR_SHAPE, 1, -1)
        assert _unchanged([d, d_ok], [bad, ok]), entry
    with pytest.raises(RuntimeError):
        O.bias_absorb(bad["w2"], bad["b1"], bad["b2"], bad["bn_w"], bad["bn_b"], 10, N_SIGMA)
    good = _relation(9950, 9, "dense", 9, 6)
    good["i2"] = 4
    good["w2"] = values(9951, 6 * 4 * 9, -26, -22).reshape(6, 4, 9)
    ob1, ob2, _, ofb = O.bias_absorb(good["w2"], good["b1"], good["b2"], good["bn_w"], good["bn_b"], 9, N_SIGMA)
    one, bat = _Dev(good), _Dev(good)
    _lib.check(_single(one), "dfq_bias_absorb")
    rc, failed, _ = _batch([bat])
    _lib.check(rc, "dfq_bias_absorb_batch")
    ref, bound, _ = _b2_reference_and_bound(good)
    for got in (one.out(), bat.out()):
        assert _bits(got["b1"], ob1) and _bits(got["bn_b"], ofb)
        assert (np.abs(got["b2"].astype(np.float64) - ref) <= bound + 2.0 ** -24 * np.abs(got["b2"])).all()
    assert _bits(one.out()["b2"], bat.out()["b2"])
