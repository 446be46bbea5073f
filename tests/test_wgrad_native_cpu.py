"""Host side of the native weight gradient (`phc_wgrad_bf16`, `+learning.params.config.wgrad=native`) where no device is needed: argument checks of
the C ABI (they return before the device is touched), the shape-only split / workspace queries, and the learner switch (validated when the
agent is built; inert off the device)."""
import pytest
import torch

from test_learner_cpu import FakeVecEnv
from phc_amd.config import compose
from phc_amd.learning.amp_agent import IMAmpAgent

PRODUCT = [(16384, 1024, 934), (16384, 1024, 1024), (12288, 1024, 1960), (12288, 1024, 2048), (16384, 512, 1024), (12288, 512, 1024), (16384, 69, 512),
           (12288, 69, 512)]


SMALL = ["learning.params.config.horizon_length=8", "learning.params.config.minibatch_size=64", "learning.params.config.mini_epochs=2",
         "learning.params.config.amp_minibatch_size=32", "learning.params.config.amp_batch_size=16", "learning.params.config.amp_obs_demo_buffer_size=256",
         "learning.params.config.amp_replay_buffer_size=256", "learning.params.network.mlp.units=[32,16]", "learning.params.network.disc.units=[32,16]"]


def _lib():
    from phc_amd import _lib as L
    return L.load()


def test_symbols_are_in_the_ctypes_table_and_the_abi_number_stays():
    from phc_amd import _lib as L
    assert {"phc_wgrad_bf16", "phc_wgrad_bf16_workspace", "phc_wgrad_bf16_slices"} <= set(L.EXPORTED_SYMBOLS)
    assert _lib().phc_abi_version() == 37


def test_invalid_arguments_return_einval_without_a_device():
    lib = _lib()
    P = 4096   # (never dereferenced: every call below is refused on the host)
    good = dict(gy=P, y=P, x=P, ld_x=8, rows=4, n=8, k=8, gw=P, ld_gw=8, acc=0, gz=P, gb=P, gbacc=0, ws=P, stream=None)

    def call(**kw):
        a = dict(good, **kw)
        return lib.phc_wgrad_bf16(a["gy"], a["y"], a["x"], a["ld_x"], a["rows"], a["n"], a["k"], a["gw"], a["ld_gw"], a["acc"], a["gz"], a["gb"], a["gbacc"],
                                  a["ws"], a["stream"])

    for bad in (dict(gy=None), dict(x=None), dict(gw=None), dict(ws=None), dict(rows=0), dict(rows=-3), dict(n=0), dict(n=-1), dict(k=0), dict(k=-8),
                dict(ld_x=7), dict(ld_x=0), dict(ld_gw=7), dict(ld_gw=-1), dict(ws=P + 8), dict(gw=P + 2), dict(gb=P + 1), dict(gy=P + 1), dict(gz=P + 1)):
        assert call(**bad) == -1, f"{bad} was not refused"
    for q in (lib.phc_wgrad_bf16_slices, lib.phc_wgrad_bf16_workspace):
        for rows, n, k in ((0, 8, 8), (8, 0, 8), (8, 8, 0), (-1, 8, 8)):
            assert q(rows, n, k) == -1


@pytest.mark.parametrize("rows,n,k", PRODUCT + [(1, 1, 1), (4099, 69, 130), (2047, 33, 5)], ids=lambda v: str(v))
def test_split_and_workspace_are_functions_of_the_shape(rows, n, k):
    lib = _lib()
    slices, nbytes = lib.phc_wgrad_bf16_slices(rows, n, k), lib.phc_wgrad_bf16_workspace(rows, n, k)
    assert slices >= 1 and nbytes > 0 and nbytes >= slices * n * k * 4
    for _ in range(3):
        assert lib.phc_wgrad_bf16_slices(rows, n, k) == slices and lib.phc_wgrad_bf16_workspace(rows, n, k) == nbytes
    assert -(-rows // slices) * (slices - 1) < rows, "an empty slice"


def _cfg(*extra):
    return compose(SMALL + list(extra))


def test_unknown_wgrad_value_raises_when_the_agent_is_built():
    with pytest.raises(ValueError, match="wgrad"):
        IMAmpAgent(FakeVecEnv(32), _cfg("+learning.params.config.wgrad=bogus"), bf16=False)


def _train(*extra):
    torch.manual_seed(0)
    agent = IMAmpAgent(FakeVecEnv(32), _cfg(*extra), bf16=False)
    agent.init_train()
    infos = [agent.train_epoch() for _ in range(2)]
    return agent, infos


def test_the_switch_is_inert_on_a_cpu_agent():
    """Two epochs with wgrad=native on the CPU equal the default run bit for bit: the tag only acts in the bf16 device pass."""
    from phc_amd.learning.fast_ops import _DeviceLinear
    a_lib, i_lib = _train("+learning.params.config.wgrad=library")
    a_def, _ = _train()
    a_nat, i_nat = _train("+learning.params.config.wgrad=native")
    assert a_nat._wgrad == "native" and a_lib._wgrad == a_def._wgrad == "library"
    tagged = [m for m in a_nat.model.modules() if isinstance(m, _DeviceLinear)]
    assert tagged and all(m.weight._wgrad_native for m in tagged)
    assert not any(getattr(m.weight, "_wgrad_native", False) for m in a_lib.model.modules() if isinstance(m, _DeviceLinear))
    for (k, p), (_, q), (_, r) in zip(a_lib.model.state_dict().items(), a_nat.model.state_dict().items(), a_def.model.state_dict().items()):
        assert torch.equal(p, q) and torch.equal(p, r), k
    for x, z in zip(i_lib, i_nat):
        for key in ("actor_loss", "critic_loss", "disc_loss", "kl"):
            assert float(x[key]) == float(z[key]), key
