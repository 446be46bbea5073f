"""`wgrad=native` at the layer and the agent level (fast_ops.set_wgrad, `+learning.params.config.wgrad=native`): the bf16 device layers form their
weight and bias gradients with ONE phc_wgrad_bf16 launch; the input gradient stays the library's GEMM on the same masked output gradient.

Layer bounds are those of tests/test_wgrad_native_gpu.py (rounding depth of the kernel's fp32 reduction, U = 2^-24) against the float64 layer on
the bf16 operands; the agent runs use the tolerances of tests/test_learner_epoch.py's bf16 test unchanged (they compare with the reference fixture)."""
import numpy as np
import pytest
import torch

import test_learner_epoch as tle
from test_learn_kernel_edges import within
from test_wgrad_native_gpu import U, _depth

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


def _layer(kind, relu, K, N, mode, seed=0):
    from phc_amd.learning import fast_ops as fo
    from phc_amd.learning.amp_agent import FlatGradBucket
    from phc_amd.learning.network import build_mlp
    torch.manual_seed(seed)
    linear = getattr(fo, kind)
    net = build_mlp(K, [N], "relu", linear).cuda() if relu else torch.nn.Sequential(linear(K, N)).cuda()
    if not relu:
        from phc_amd.learning.network import pad_cols
        net[0].weight._pad_cols = pad_cols(K)      # (what build_mlp does for a first layer)
    fo.set_wgrad(net, mode)
    return net, FlatGradBucket(net.parameters())


def _pass(net, bucket, xs, cots, defer=True):
    """One backward pass of sum_i <net(x_i), cot_i> -> (input gradients, flat parameter gradient, layer outputs)"""
    from phc_amd.learning import fast_ops as fo
    xs = [x.clone().requires_grad_(True) for x in xs]
    with bucket.shadow_scope():
        bucket.zero()
        with torch.autocast("cuda", dtype=BF):
            ys = [net(x) for x in xs]
        loss = sum((y.float() * c).sum() for y, c in zip(ys, cots))
        if defer:
            with fo.deferred_colsums():
                loss.backward()
        else:
            loss.backward()
        assert not fo._pending and not fo._pending_dst
    torch.cuda.synchronize()
    return [x.grad.clone() for x in xs], bucket.flat.clone(), [y.detach() for y in ys]


class _counting:
    """Counts the calls of the gradient kernels' host wrappers in fast_ops while the block runs."""
    NAMES = ("wgrad_native", "wgrad_split_k", "colsum_bf16", "colsum_relu_bf16")

    def __init__(self, monkeypatch):
        self.mp = monkeypatch

    def __enter__(self):
        from phc_amd.learning import fast_ops as fo
        counts = dict.fromkeys(self.NAMES, 0)
        self.ctx = self.mp.context()
        m = self.ctx.__enter__()
        for name in self.NAMES:
            def wrapped(*a, _f=getattr(fo, name), _n=name, **kw):
                counts[_n] += 1
                return _f(*a, **kw)
            m.setattr(fo, name, wrapped)
        return counts

    def __exit__(self, *exc):
        return self.ctx.__exit__(*exc)


def _segment(bucket, p, flat):
    o, k = bucket.segments[[id(q) for q in bucket.params].index(id(p))]
    return flat[o:o + k]


LAYERS = [(4096, 934, 1024), (4096, 512, 69), (1000, 130, 7)]     # (rows, K, N): a K-padded first layer, an aligned layer, a small odd one


@pytest.mark.parametrize("rows,K,N", LAYERS, ids=lambda v: str(v))
@pytest.mark.parametrize("relu", [False, True], ids=["plain", "fused_relu"])
@pytest.mark.parametrize("kind", ["FastLinear", "FastLinearDD"])
def test_layer_gradients(kind, relu, rows, K, N, monkeypatch):
    """gx bit-identical to wgrad=library; weight / bias gradients within the kernel's rounding bound of the float64 layer on the bf16 operands; the
    native launch really served the layer (no slab-sum / column-sum job of the library path is left pending, and a K-padded weight's pad columns
    stay zero)."""
    from phc_amd.learning.network import pad_cols
    g = torch.Generator().manual_seed(rows + K + N)
    Kp = pad_cols(K) or K
    x = torch.zeros(rows, Kp)
    x[:, :K] = torch.relu(torch.randn(rows, K, generator=g))
    x = x.cuda()
    cot = (0.01 * torch.randn(rows, N, generator=g)).cuda()
    out, calls = {}, {}
    for mode in ("library", "native"):
        net, bucket = _layer(kind, relu, K, N, mode)
        with _counting(monkeypatch) as calls[mode]:
            out[mode] = (net, bucket) + _pass(net, bucket, [x], [cot])
    assert calls["native"] == dict(wgrad_native=1, wgrad_split_k=0, colsum_bf16=0, colsum_relu_bf16=0), calls["native"]
    assert calls["library"]["wgrad_native"] == 0 and calls["library"]["wgrad_split_k"] == 1, calls["library"]
    (net_l, _, gx_l, _, y_l), (net, bucket, gx_n, flat, y_n) = out["library"], out["native"]
    assert torch.equal(y_l[0], y_n[0])
    assert torch.equal(gx_l[0].view(torch.int32 if gx_l[0].dtype == torch.float32 else torch.int16),
                       gx_n[0].view(torch.int32 if gx_n[0].dtype == torch.float32 else torch.int16)), "the input gradient differs from the library path"
    lin = net[0]
    # the float64 layer on the bf16 operands
    xb = x[:, :K].to(BF).double().cpu().numpy()
    gz = cot.to(BF).double().cpu().numpy()
    if relu:
        gz = np.where(y_n[0].double().cpu().numpy() > 0, gz, 0.0)
    kk = Kp if getattr(lin.weight, "_grad_padded", None) is not None else K
    depth = _depth(rows, N, kk)
    gw_ref, gw_abs = gz.T @ xb, np.abs(gz).T @ np.abs(xb)
    gw = lin.weight.grad.double().cpu().numpy()
    within(gw, gw_ref, depth * U * gw_abs + U * np.abs(gw_ref), "weight gradient")
    gb_ref = gz.sum(0)
    within(lin.bias.grad.double().cpu().numpy(), gb_ref, depth * U * np.abs(gz).sum(0) + U * np.abs(gb_ref), "bias gradient")
    gp = getattr(lin.weight, "_grad_padded", None)
    if gp is not None:
        assert float(gp[:, K:].abs().max()) == 0.0, "pad columns of a K-padded weight gradient must stay zero"
    # and the library path on the same data is the bf16-slab path: close, not equal (the test would show nothing if both ran the same kernels)
    gw_l = net_l[0].weight.grad.double().cpu().numpy()
    assert np.abs(gw_l - gw_ref).max() <= 2e-2 * np.abs(gw_ref).max()


@pytest.mark.parametrize("kind", ["FastLinear", "FastLinearDD"])
@pytest.mark.parametrize("defer", [True, False], ids=["deferred_colsums", "immediate"])
def test_a_layer_applied_twice_accumulates_both_contributions(kind, defer):
    """The second application of a layer in one pass ADDS to what the first one stored, weight and bias alike: since the kernel is deterministic and the
    accumulate is one fp32 add of the finished sum, the result equals the fp32 sum of two separate passes bit for bit."""
    rows, K, N = 4096, 96, 64
    g = torch.Generator().manual_seed(7)
    xa, xb = torch.relu(torch.randn(rows, K, generator=g)).cuda(), (torch.randn(rows, K, generator=g) * 0.5 + 0.3).cuda()
    ca, cb = (0.01 * torch.randn(rows, N, generator=g)).cuda(), (0.02 * torch.randn(rows, N, generator=g)).cuda()
    net, bucket = _layer(kind, True, K, N, "native")
    _, fa, _ = _pass(net, bucket, [xa], [ca], defer)
    _, fb, _ = _pass(net, bucket, [xb], [cb], defer)
    _, both, _ = _pass(net, bucket, [xa, xb], [ca, cb], defer)
    for p in (net[0].weight, net[0].bias):
        want, got = _segment(bucket, p, fa) + _segment(bucket, p, fb), _segment(bucket, p, both)
        assert float(want.abs().max()) > 0
        assert torch.equal(want.view(torch.int32), got.view(torch.int32)), tuple(p.shape)


def test_discriminator_pattern_with_gradient_penalty_stays_close_to_the_library_path():
    """FastLinearDD under loss + gradient penalty (the double backward keeps its own path; the first-order pass is native): parameter gradients agree with
    wgrad=library within bf16 GEMM accuracy (2e-2 of each gradient's scale, the bound tests/test_learn_gpu.py uses between bf16 paths)."""
    from phc_amd.learning import fast_ops as fo
    from phc_amd.learning.amp_agent import FlatGradBucket
    from phc_amd.learning.network import build_mlp
    rows, K = 3 * 1024, 130
    g = torch.Generator().manual_seed(3)
    x = torch.randn(rows, K, generator=g).cuda()
    flats = {}
    for mode in ("library", "native"):
        torch.manual_seed(1)
        net = torch.nn.Sequential(build_mlp(K, [256, 128], "relu", fo.FastLinearDD), fo.FastLinearDD(128, 64)).cuda()
        fo.set_wgrad(net, mode)
        bucket = FlatGradBucket(net.parameters())
        with bucket.shadow_scope():
            bucket.zero()
            xin = x.clone().requires_grad_(True)
            with torch.autocast("cuda", dtype=BF):
                out = net(xin)
                gx, = torch.autograd.grad(out.float().sum(), xin, create_graph=True)
                loss = (out.float() ** 2).mean() + 5.0 * gx.float().pow(2).sum(-1).mean()
            with fo.deferred_colsums():
                loss.backward()
        torch.cuda.synchronize()
        flats[mode] = (bucket, bucket.flat.clone())
    (bl, fl), (bn, fn) = flats["library"], flats["native"]
    for (o, k) in bl.segments:
        scale = float(fl[o:o + k].abs().max())
        assert scale > 0 and float((fl[o:o + k] - fn[o:o + k]).abs().max()) <= 2e-2 * scale


# ---- the agent -------------------------------------------------------------------------------------------------------------------------------
BF16_TOL = dict(exp=2e-4, net=3e-2, nlp=2.0, scal_r=0.15, scal_a=2e-3, stat=2e-6, stat_a=1e-7, vstat=5e-2, param_mean=0.35, count_slack=6.0 / 32,
                skip_scalars=("actor_loss", "kl"))     # (test_three_epochs_of_the_reference_agent_on_hip_with_bf16_gemms, unchanged)


def _epochs(golden, monkeypatch, graph):
    agents = []

    class Recording(tle.IMAmpAgent):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            agents.append(self)

    monkeypatch.setattr(tle, "IMAmpAgent", Recording)
    extra = ["+learning.params.config.hip_graph=True", "+learning.params.config.hip_graph_min_rows=1"] if graph else ["+learning.params.config.hip_graph=False"]
    with _counting(monkeypatch) as calls:
        worst = tle.run_epochs(golden("learner_epoch"), "cuda", extra=extra + ["+learning.params.config.wgrad=native"], graphs=graph, bf16=True, tol=BF16_TOL)
    torch.cuda.synchronize()
    assert len(agents) == 1 and agents[0]._wgrad == "native"
    assert calls["wgrad_native"] > 0 and calls["colsum_relu_bf16"] == 0, calls     # (the fused-ReLU layers are all served by the native launch)
    print(f"wgrad=native graph={graph}: worst mean parameter error / mean update over the three epochs = {worst:.3f}")
    return {k: v.detach().clone() for k, v in agents[0].model.state_dict().items()}


def test_three_epochs_of_the_reference_agent_with_native_wgrad_eager_and_graph(golden, monkeypatch):
    """tests/test_learner_epoch.py's bf16 run with wgrad=native, launched eagerly and replayed from hipGraphs, at that test's tolerances; the two runs end
    with bit-identical parameters."""
    eager = _epochs(golden, monkeypatch, graph=False)
    graph = _epochs(golden, monkeypatch, graph=True)
    for k in eager:
        assert torch.equal(eager[k], graph[k]), f"{k}: eager and graph runs differ"


def _im_run():
    from test_env_gpu import make_task
    from phc_amd.learning.amp_agent import IMAmpAgent
    task, env = make_task(256, motion="synthetic:2:3", seed=4, **{"learning.params.config.minibatch_size": 2048,
                                                                 "learning.params.config.amp_obs_demo_buffer_size": 4096,
                                                                 "learning.params.config.amp_replay_buffer_size": 4096,
                                                                 "+learning.params.config.wgrad": "native"})
    torch.manual_seed(4)
    agent = IMAmpAgent(env, task.cfg)
    assert agent._wgrad == "native" and agent.bf16
    agent.init_train()
    infos = [agent.train_epoch() for _ in range(2)]
    torch.cuda.synchronize()
    assert np.isfinite([infos[-1]["actor_loss"], infos[-1]["critic_loss"], infos[-1]["disc_loss"]]).all()
    return {k: v.detach().clone() for k, v in agent.model.state_dict().items()}


def test_seeded_im_training_is_bit_reproducible_with_native_wgrad():
    a, b = _im_run(), _im_run()
    moved = False
    for k in a:
        assert torch.equal(a[k], b[k]), f"{k}: two executions of the same seeded run differ"
        moved = moved or bool((a[k] != 0).any())
    assert moved
