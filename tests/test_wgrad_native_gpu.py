"""The native bf16 weight-gradient kernel (csrc/phc_gemm.hip, `phc_wgrad_bf16`) through the C ABI, against a float64 numpy statement of

    gz[r, j]  = y is None ? gy[r, j] : (y[r, j] > 0 ? gy[r, j] : 0)
    gw[j, c] (=|+=) sum_r gz[r, j] * x[r, c]
    gb[j]    (=|+=) sum_r gz[r, j]

Every output sits inside sentinel padding (`Buf` of tests/test_learn_kernel_edges.py), also between the rows of a strided gw, and the
sentinels must be bit-unchanged after each call.

Tolerances are rounding bounds, U = 2^-24 (fp32 unit round-off); nothing here is fitted to what the kernel returns.
* gz is a select: bit-exact.
* gw: |got - ref| <= depth * U * (|gz|^T |x|) + U * |ref|, where `depth` is the largest number of fp32 roundings a product passes through:
  16 (inside one 32x32x16 MFMA, whatever its internal order) + the MFMA steps of a slice, ceil(rows_per_slice / 16) with
  rows_per_slice = ceil(rows / slices) + slices (the slabs added in order) + 1 (the accumulate).  The products themselves are exact in fp32
  (8 x 8 significant bits).  `slices` is asked from phc_wgrad_bf16_slices, not assumed.
* gb: the same with |gz| summed over the rows; its reduction is a per-thread running sum over every 16th row of the slice (ceil(rows_per_slice / 16)
  adds), 16 of those added in order, then the slices and the accumulate: the same depth.
A path that rounds a partial sum to bf16 on the way (the library path's slabs) exceeds this bound by more than an order of magnitude.
"""
import numpy as np
import pytest
import torch

from test_learn_kernel_edges import Buf, within

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
BF = torch.bfloat16


def _lib():
    from phc_amd import _lib as L
    return L.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _inputs(rows, n, k, seed):
    """gy ~ 0.01 N(0, 1), x = relu(N(0, 1)), y = relu(N(0, 1)) with exact zeros (about half) and some negative zeros, all rounded to bf16"""
    g = torch.Generator().manual_seed(seed)
    gy = (0.01 * torch.randn(rows, n, generator=g)).to(BF)
    x = torch.relu(torch.randn(rows, k, generator=g)).to(BF)
    y = torch.relu(torch.randn(rows, n, generator=g)).to(BF)
    neg = torch.rand(rows, n, generator=g) < 0.1
    y = torch.where(neg & (y == 0), torch.tensor(-0.0, dtype=BF), y)
    return gy, y, x


def _view(t, offset, ld=None):
    """A device copy of the 2-D tensor `t` as a view `offset` elements into a larger allocation, rows `ld` elements apart."""
    rows, cols = t.shape
    ld = ld or cols
    base = torch.full((offset + rows * ld + 8,), 7.0, dtype=t.dtype, device="cuda")   # (7: a pad column that is read shows up in the result)
    v = base[offset:offset + rows * ld].view(rows, ld)[:, :cols]
    v.copy_(t)
    return v


def _reference(gy, y, x):
    gz = gy.double().numpy()
    if y is not None:
        gz = np.where(y.double().numpy() > 0, gz, 0.0)
    xd = x.double().numpy()
    return gz, gz.T @ xd, gz.sum(0), np.abs(gz).T @ np.abs(xd), np.abs(gz).sum(0)


def _depth(rows, n, k):
    slices = _lib().phc_wgrad_bf16_slices(rows, n, k)
    assert slices >= 1
    rows_per_slice = -(-rows // slices)
    return 16 + -(-rows_per_slice // 16) + slices + 1


def _workspace(rows, n, k):
    nbytes = _lib().phc_wgrad_bf16_workspace(rows, n, k)
    assert nbytes >= _lib().phc_wgrad_bf16_slices(rows, n, k) * n * k * 4
    return torch.full((nbytes,), 0xA5, dtype=torch.uint8, device="cuda")   # (garbage: the call zeroes its own tickets)


def _run_case(rows, n, k, seed, ld_x=None, mask=True, want_gz=True, want_gb=True, accumulate=False, off=(0, 0, 0, 0, 0), ld_gw=None, what=""):
    """One call, every output checked.  off: element offsets of (gy, y, x, gz, gw) inside their allocations."""
    lib = _lib()
    gy, y, x = _inputs(rows, n, k, seed)
    if not mask:
        y = None
    gz_ref, gw_ref, gb_ref, gw_abs, gb_abs = _reference(gy, y, x)
    gyd = _view(gy, off[0])
    yd = _view(y, off[1]) if mask else None
    xd = _view(x, off[2], ld_x)
    ld_gw = ld_gw or k
    g = torch.Generator().manual_seed(seed + 1)
    gw0 = torch.randn(n, k, generator=g) if accumulate else None
    gb0 = torch.randn(n, generator=g) if accumulate else None
    gw = Buf((n, k), torch.float32, offset=off[4], stride=ld_gw, init=gw0)
    gb = Buf(n, torch.float32, offset=1, init=gb0) if want_gb else None
    gz = Buf((rows, n), BF, offset=off[3]) if want_gz else None
    ws = _workspace(rows, n, k)
    rc = lib.phc_wgrad_bf16(gyd.data_ptr(), yd.data_ptr() if mask else None, xd.data_ptr(), xd.stride(0), rows, n, k, gw.ptr, ld_gw, int(accumulate),
                            gz.ptr if want_gz else None, gb.ptr if want_gb else None, int(accumulate), ws.data_ptr(), _stream())
    assert rc == 0, what
    torch.cuda.synchronize()
    depth = _depth(rows, n, k)
    if accumulate:
        gw_ref = gw0.double().numpy() + gw_ref
        gb_ref = gb0.double().numpy() + gb_ref
    gw.check(what + " gw")
    within(gw.np(), gw_ref, depth * U * gw_abs + U * np.abs(gw_ref), what + " gw")
    if want_gb:
        gb.check(what + " gb")
        within(gb.np(), gb_ref, depth * U * gb_abs + U * np.abs(gb_ref), what + " gb")
    if want_gz:
        gz.check(what + " gz")
        expect = torch.from_numpy(gz_ref).to(BF)     # (exact: every value is a bf16 number or +0)
        assert torch.equal(gz.t.cpu().view(torch.int16), expect.view(torch.int16)), what + " gz is not the exact select"
    return gw, gb


# ---- the product shapes ---------------------------------------------------------------------------------------------------------------
PRODUCT = [(16384, 1024, 934, 1024), (16384, 1024, 934, 934), (12288, 1024, 1960, 2048), (12288, 1024, 1960, 1960), (16384, 1024, 1024, 1024),
           (12288, 1024, 2048, 2048), (16384, 512, 1024, 1024), (12288, 512, 1024, 1024), (16384, 69, 512, 512), (12288, 69, 512, 512)]


@pytest.mark.parametrize("rows,n,k,ld_x", PRODUCT, ids=lambda v: str(v))
def test_product_shapes(rows, n, k, ld_x):
    """Actor / critic (16384 rows) and discriminator (12288 rows) layers, first layers K-padded (ld_x 1024 / 2048: the pad columns are not read into
    the result) and unpadded (PHC_NO_K_PAD=1): masked with every side output, stored; then unmasked, no side outputs, accumulated onto a non-zero gw."""
    _run_case(rows, n, k, seed=rows + n + k, ld_x=ld_x, what=f"{rows}x{n}x{k} store")
    _run_case(rows, n, k, seed=rows + n + k + 7, ld_x=ld_x, mask=False, want_gz=False, want_gb=False, accumulate=True, ld_gw=k + 3,
              what=f"{rows}x{n}x{k} accumulate")


# ---- edges ----------------------------------------------------------------------------------------------------------------------------
ROWS = [1, 15, 16, 17, 63, 64, 65, 2047, 4099]
NS = [1, 7, 32, 33, 69]
KS = [(1, 1), (5, 5), (130, 130), (934, 934), (934, 942), (934, 1024)]    # (k, ld_x)
OFFSETS = [(0, 0, 0, 0, 0), (1, 1, 1, 1, 1), (8, 8, 8, 8, 4), (3, 0, 8, 5, 2), (0, 8, 1, 0, 3)]


@pytest.mark.parametrize("rows", ROWS, ids=lambda r: f"rows{r}")
def test_edge_shapes(rows):
    """rows x n x (k, ld_x) over the tile, stage, slice and vector-path boundaries; the switches (mask, gz, gb, accumulate), the operand offsets and a
    strided gw cycle so that every value of each is met with every rows and every n (the counter runs over 30 cases per rows; the cycles have
    lengths 16 and 5, so all 80 combinations of switches and offsets appear across the rows)."""
    i = ROWS.index(rows) * 7
    for n in NS:
        for k, ld_x in KS:
            sw = i % 16
            _run_case(rows, n, k, seed=1000 * rows + 10 * n + k, ld_x=ld_x, mask=bool(sw & 1), want_gz=bool(sw & 2), want_gb=bool(sw & 4),
                      accumulate=bool(sw & 8), off=OFFSETS[i % 5], ld_gw=k + (i % 3) * 5, what=f"rows {rows} n {n} k {k} ld_x {ld_x} case {i}")
            i += 1


def test_every_switch_at_one_sliced_shape():
    """All 16 switch settings where the row split is active (4099 rows: 8 slices), aligned and offset."""
    assert _lib().phc_wgrad_bf16_slices(4099, 69, 130) > 1
    for sw in range(16):
        for off in (OFFSETS[0], OFFSETS[3]):
            _run_case(4099, 69, 130, seed=sw, mask=bool(sw & 1), want_gz=bool(sw & 2), want_gb=bool(sw & 4), accumulate=bool(sw & 8), off=off,
                      ld_gw=133, what=f"switches {sw} offsets {off}")


# ---- reproducibility --------------------------------------------------------------------------------------------------------------------
def _call(dev, gw, gb, ws, rows, n, k, accumulate=0, gz=None):
    gyd, yd, xd = dev
    rc = _lib().phc_wgrad_bf16(gyd.data_ptr(), yd.data_ptr(), xd.data_ptr(), xd.stride(0), rows, n, k, gw.data_ptr(), k, accumulate,
                               None if gz is None else gz.data_ptr(), gb.data_ptr(), accumulate, ws.data_ptr(), _stream())
    assert rc == 0


REPRO = [(16384, 512, 1024), (4099, 69, 130), (12288, 1024, 2048)]


@pytest.mark.parametrize("rows,n,k", REPRO, ids=lambda v: str(v))
def test_bit_identical_between_calls_and_under_graph_replay(rows, n, k):
    dev = [t.cuda() for t in _inputs(rows, n, k, seed=5)]
    ws = _workspace(rows, n, k)
    outs = []
    for _ in range(3):
        gw = torch.full((n, k), float("nan"), device="cuda")
        gb = torch.full((n,), float("nan"), device="cuda")
        _call(dev, gw, gb, ws, rows, n, k)
        torch.cuda.synchronize()
        outs.append((gw.clone(), gb.clone()))
    for gw, gb in outs[1:]:
        assert torch.equal(gw.view(torch.int32), outs[0][0].view(torch.int32)) and torch.equal(gb.view(torch.int32), outs[0][1].view(torch.int32))
    # the same call captured and replayed (twice: the tickets are zeroed by a node of the graph, not by the host)
    gw = torch.full((n, k), float("nan"), device="cuda")
    gb = torch.full((n,), float("nan"), device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        _call(dev, gw, gb, ws, rows, n, k)      # (warm-up on the capture stream)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _call(dev, gw, gb, ws, rows, n, k)
    for _ in range(2):
        gw.fill_(float("nan"))
        gb.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(gw.view(torch.int32), outs[0][0].view(torch.int32)), "graph replay differs from the eager call"
        assert torch.equal(gb.view(torch.int32), outs[0][1].view(torch.int32)), "graph replay differs from the eager call (gb)"


def test_two_streams_with_their_own_workspaces():
    """Two different products in flight on two streams, each with its own workspace: both equal their solitary runs bit for bit."""
    shapes = [(16384, 512, 1024), (12288, 1024, 934)]
    devs = [[t.cuda() for t in _inputs(*s, seed=11 + i)] for i, s in enumerate(shapes)]
    wss = [_workspace(*s) for s in shapes]
    alone = []
    for dev, ws, (rows, n, k) in zip(devs, wss, shapes):
        gw, gb = torch.empty(n, k, device="cuda"), torch.empty(n, device="cuda")
        _call(dev, gw, gb, ws, rows, n, k)
        torch.cuda.synchronize()
        alone.append((gw, gb))
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs = [(torch.empty(n, k, device="cuda"), torch.empty(n, device="cuda")) for _, n, k in shapes]
    torch.cuda.synchronize()
    for rep in range(4):
        for st, dev, ws, (rows, n, k), (gw, gb) in zip(streams, devs, wss, shapes, outs):
            with torch.cuda.stream(st):
                _call(dev, gw, gb, ws, rows, n, k)
    torch.cuda.synchronize()
    for (gw, gb), (gw1, gb1) in zip(outs, alone):
        assert torch.equal(gw.view(torch.int32), gw1.view(torch.int32)) and torch.equal(gb.view(torch.int32), gb1.view(torch.int32))
