"""What the GPU tests of mx.mx_quantize share (test_gpu_mx.py, test_gpu_mx6.py,
test_gpu_mx_search.py): every tensor of a case placed inside a larger buffer of guard
words, one call over a list of cases with every buffer brought back whole, and the
comparison of a floor-rule case with its numpy statement, guards included.  A case is a
Case of tests/mx_cases.py, mx6_cases.py or mx_search_cases.py; ``code_offset`` (the
bytes of the codes past a 4-B boundary) is 0 where the case has none."""
import numpy as np
import torch

from tests import mx6_cases as M6
from tests import mx_cases as MC

GUARD = 16   # elements after every output
GF, GB = 12345.0, 0xA5
FORMATS = {**MC.FORMATS, **M6.FORMATS}


def place(a, dev, off):
    """``a`` on the device, starting ``off`` floats into a larger (aligned) buffer."""
    buf = torch.full((a.size + 8 + GUARD,), GF, dtype=torch.float32, device=dev)
    v = buf[off:off + a.size].view(a.shape)
    v.copy_(torch.from_numpy(np.array(a)))   # a copy: the cases are read-only
    assert v.is_contiguous() and v.data_ptr() % 16 == 4 * off
    return buf, v


def items(cases, dev):
    from data_free_quantization_amd import mx
    items, bufs = [], []
    for c in cases:
        rows, row_len = c.x.shape
        nb, cb = MC.blocks(row_len), FORMATS[c.fmt][3]
        co = getattr(c, "code_offset", 0)
        sbuf, src = place(c.x, dev, c.offset)
        b = {"src": sbuf}
        it = mx.MXItem(src=src, fmt=c.fmt, khw=c.khw, rows=rows)
        if c.outputs == "inplace":
            it.dst, b["dst"] = src, sbuf
        elif c.want_dst:
            b["dst"] = torch.full((c.x.size + 8 + GUARD,), GF, dtype=torch.float32, device=dev)
            it.dst = b["dst"][c.offset:c.offset + c.x.size].view(c.x.shape)
        if c.want_codes:
            b["codes"] = torch.full((co + rows * nb * cb + GUARD,), GB, dtype=torch.uint8, device=dev)
            b["scales"] = torch.full((rows * nb + GUARD,), GB, dtype=torch.uint8, device=dev)
            it.codes, it.scales = b["codes"][co:co + rows * nb * cb], b["scales"][:rows * nb]
            assert it.codes.data_ptr() % 4 == co
        if c.want_esum:
            b["esum"] = torch.full((c.x.size // c.khw + GUARD,), GF, dtype=torch.float32, device=dev)
            it.esum = b["esum"][:c.x.size // c.khw]
        items.append(it)
        bufs.append(b)
    return items, bufs


def run(cases, scale_search=False):
    """One call over ``cases``; every buffer back on the host, guards included."""
    from data_free_quantization_amd import mx
    its, bufs = items(cases, torch.device("cuda:0"))
    mx.mx_quantize(its, scale_search=scale_search)
    torch.cuda.synchronize()
    return [{k: v.cpu().numpy() for k, v in b.items()} for b in bufs]


def as_bytes(out):
    return {k: v.tobytes() for k, v in out.items()}


def check(c, out):
    """A floor-rule case against its statement: every output for equality, every guard word
    before and after it untouched."""
    rows, row_len = c.x.shape
    n, off = c.x.size, c.offset
    nb, cb = MC.blocks(row_len), FORMATS[c.fmt][3]
    co = getattr(c, "code_offset", 0)
    assert set(out) == {"src"} | ({"dst"} if c.want_dst else set()) | \
        ({"codes", "scales"} if c.want_codes else set()) | ({"esum"} if c.want_esum else set()), c.name
    if c.want_codes:
        assert np.array_equal(out["codes"][co:co + rows * nb * cb].reshape(rows, nb, cb), c.ref["codes"]), c.name
        assert np.array_equal(out["scales"][:rows * nb].reshape(rows, nb), c.ref["scales"]), c.name
        assert (out["codes"][:co] == GB).all() and (out["codes"][co + rows * nb * cb:] == GB).all(), c.name
        assert (out["scales"][rows * nb:] == GB).all(), c.name
    if c.want_dst:
        y = out["dst"][off:off + n].reshape(c.x.shape)
        assert np.array_equal(y.view(np.uint32), c.ref["y"].view(np.uint32)), c.name
        assert (out["dst"][:off] == GF).all() and (out["dst"][off + n:] == GF).all(), c.name
    if c.outputs != "inplace":   # the source is only read
        assert np.array_equal(out["src"][off:off + n].view(np.uint32), c.x.reshape(-1).view(np.uint32)), c.name
        assert (out["src"][:off] == GF).all() and (out["src"][off + n:] == GF).all(), c.name
    if c.want_esum:
        ne = n // c.khw
        assert np.array_equal(out["esum"][:ne], MC.esum_reference(c)), c.name
        assert (out["esum"][ne:] == GF).all(), c.name
