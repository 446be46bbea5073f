"""Helpers of tests/test_distill_gpu.py: device buffers inside sentinel-filled allocations (the helper of tests/test_learn_kernel_edges.py, copied: test
modules are not imported from each other) and the shared trainer fixture."""
import numpy as np
import torch

U = 2.0 ** -24          # fp32 unit round-off
UB = 2.0 ** -8          # bf16 unit round-off (8 significant bits: half an ulp is 2^-8 of the binade's start)
PAD = 64                # sentinel elements on each side of a buffer
_INT = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float64: torch.int64, torch.int64: torch.int64}
_SENT = {torch.float32: 0x7FC0BAD1, torch.bfloat16: 0x7FB1, torch.float64: 0x7FF8DEADBEEF0001, torch.int64: 0x7FF8DEADBEEF0001}


def lib():
    from phc_amd import _lib as L
    return L.load()


def stream():
    return torch.cuda.current_stream().cuda_stream


class Buf:
    """A [n] or [rows, cols] device tensor inside a sentinel-filled allocation: `offset` elements after PAD sentinels, rows `stride` elements
    apart, PAD sentinels after it.  `init` (None: the sentinel itself, so an element the kernel does not write shows up as NaN)."""

    def __init__(self, shape, dtype, offset=0, stride=None, init=None):
        shape = (shape,) if isinstance(shape, int) else tuple(shape)
        rows, cols = (1, shape[0]) if len(shape) == 1 else shape
        stride = stride or cols
        self.dtype, self.start, span = dtype, PAD + offset, rows * stride
        start = self.start
        self.base = torch.empty(start + span + PAD, dtype=dtype, device="cuda")
        self.base.view(_INT[dtype]).fill_(_SENT[dtype])
        region = self.base[start:start + span].view(rows, stride)[:, :cols]
        self.t = region.reshape(-1) if len(shape) == 1 else region       # (a view in both cases)
        self.outside = torch.ones(self.base.numel(), dtype=torch.bool, device="cuda")
        self.outside[start:start + span].view(rows, stride)[:, :cols] = False
        if init is not None:
            self.t.copy_(torch.as_tensor(init).reshape(self.t.shape))
        self.guard = self.base.view(_INT[dtype])[self.outside].clone()

    @property
    def ptr(self):      # (from the allocation: an empty view's data_ptr() is NULL)
        return self.base.data_ptr() + self.start * self.base.element_size()

    def np(self):
        return self.t.double().cpu().numpy() if self.dtype != torch.int64 else self.t.cpu().numpy()

    def bits(self):
        return self.t.contiguous().view(_INT[self.dtype]).clone()

    def check(self, what=""):
        assert torch.equal(self.base.view(_INT[self.dtype])[self.outside], self.guard), f"{what}: write outside the buffer"


def within(got, ref, tol, what):
    """|got - ref| <= tol elementwise (NaN only where the reference is NaN)."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    tol = np.broadcast_to(np.asarray(tol, dtype=np.float64), ref.shape)
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan), f"{what}: NaN pattern differs"
    err = np.abs(got - ref)[~nan]
    bad = err > tol[~nan]
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} beyond tolerance, worst {float((err - tol[~nan]).max()):.3g} over"


def trainer_fixture(rows, obs_dim, act_dim, seed=0):
    """A small regression problem with an observation column far outside +-5 sigma: -> dict(obs, clean_action, running_mean, running_var) as numpy / torch."""
    g = np.random.default_rng(seed)
    obs = g.standard_normal((rows, obs_dim)).astype(np.float32) * 2.0 + 0.5
    obs[3, 1] = 40.0        # > 5 sigma of the statistics below: the clamp acts
    obs[7, 2] = -35.0
    w = g.standard_normal((obs_dim, act_dim)).astype(np.float32) * 0.3
    act = np.tanh(obs.clip(-6, 6) @ w).astype(np.float32)
    mean = torch.as_tensor(g.standard_normal(obs_dim) * 0.1 + 0.5, dtype=torch.float64)
    var = torch.as_tensor(g.uniform(2.0, 5.0, obs_dim), dtype=torch.float64)
    return dict(obs=obs, clean_action=act, running_mean=mean, running_var=var)


def adam_steps(state_a, state_b, lr):
    """Largest parameter difference between two state dicts in units of lr (one Adam step moves a parameter by at most ~lr)."""
    return max(float((state_a[k].double() - state_b[k].double()).abs().max()) for k in state_a) / lr
