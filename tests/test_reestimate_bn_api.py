"""BatchNorm momentum=None through the facade's descriptor, and avmoe_amd.train.reestimate_bn on a pure-torch model: bit-equal to
torch.optim.swa_utils.update_bn, flags and momenta restored (also when a batch raises), the argument checks of `ema=` before anything
is written.  CPU only: MoEAdapter._desc only builds the struct."""
import contextlib
import copy

import pytest
import torch

from avmoe_amd import _capi as capi
from avmoe_amd.train import reestimate_bn
from oracle import avmoe_oracle as O
from tests.test_adapters_api import build_module


def _site():
    cfg = O.AdapterConfig(Cx=64, Nx=50, Cy=48, Ny=20, reduction=4, groups=2, K=6)
    return build_module("ave", cfg), cfg


def _bns(site):
    return [m for m in site.modules() if isinstance(m, torch.nn.BatchNorm2d)]


def test_the_library_declares_the_cumulative_average_and_keeps_its_abi_version():
    assert "avmoe_bn_cumulative_supported" in capi.exported_symbols()
    L = capi.lib()
    assert L.avmoe_abi_version() == 11
    assert L.avmoe_bn_cumulative_supported() == 1 and L.avmoe_bn_cumulative is True


def test_desc_takes_momentum_none_as_minus_one_and_numbers_as_before():
    site, cfg = _site()
    assert len(_bns(site)) == 2 * cfg.E
    assert site._desc(4, cfg.Nx, cfg.Ny, False).bn_momentum == pytest.approx(0.1)
    for m in _bns(site):
        m.momentum = 0.25
    assert site._desc(4, cfg.Nx, cfg.Ny, False).bn_momentum == 0.25
    for m in _bns(site):
        m.momentum = None
    assert site._desc(4, cfg.Nx, cfg.Ny, False).bn_momentum == -1.0
    assert site._desc(4, cfg.Nx, cfg.Ny, True).bn_momentum == -1.0
    for m in _bns(site):                                   # set and restored between calls (update_bn): no refresh() needed
        m.momentum = 0.1
    assert site._desc(4, cfg.Nx, cfg.Ny, False).bn_momentum == pytest.approx(0.1)


def test_desc_refuses_a_mix_of_none_and_numbers_and_a_missing_counter():
    site, cfg = _site()
    site.singlemodal_experts[1].bn2.momentum = None        # not the first expert's bn1: every BatchNorm of the site is looked at
    with pytest.raises(capi.AvmoeError) as e:
        site._desc(4, cfg.Nx, cfg.Ny, False)
    assert "singlemodal_experts.1.bn2" in str(e.value) and "multimodal_experts.0.bn1" in str(e.value)
    for m in _bns(site):
        m.momentum = None
    site.multimodal_experts[1].bn1._buffers["num_batches_tracked"] = None
    with pytest.raises(capi.AvmoeError) as e:
        site._desc(4, cfg.Nx, cfg.Ny, False)
    assert "multimodal_experts.1.bn1" in str(e.value) and "num_batches_tracked" in str(e.value)


# ---- reestimate_bn on a pure-torch model --------------------------------------------------------------------------------------
class Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.conv = torch.nn.Conv2d(3, 5, 3)
        self.bn2d = torch.nn.BatchNorm2d(5, momentum=0.3)
        self.fc = torch.nn.Linear(5, 7)
        self.bn1d = torch.nn.BatchNorm1d(7)
        self.drop = torch.nn.Dropout(0.0)

    def forward(self, x):
        return self.drop(self.bn1d(self.fc(self.bn2d(self.conv(x)).mean(dim=(2, 3)))))


def _net(train_steps=2):
    torch.manual_seed(0)
    net = Net()
    g = torch.Generator().manual_seed(3)
    for _ in range(train_steps):                           # statistics and counters away from their reset values
        net(torch.randn(6, 3, 8, 8, generator=g))
    return net


def _batches(n=5):
    g = torch.Generator().manual_seed(11)
    return [torch.randn(4, 3, 8, 8, generator=g) for _ in range(n)]


def test_reestimate_bn_equals_torch_update_bn_bit_for_bit():
    net = _net().eval()
    net.bn1d.train()                                       # a module whose flag differs from the model's: each flag is restored, not one
    ref = copy.deepcopy(net)
    torch.optim.swa_utils.update_bn([(b,) for b in _batches()], ref)      # (update_bn passes batch[0])
    ptrs = {k: v.data_ptr() for k, v in net.named_buffers()}
    assert reestimate_bn(net, _batches()) == 5
    for (k, v), (_, r) in zip(net.named_buffers(), ref.named_buffers()):
        assert torch.equal(v, r), k
    assert int(net.bn2d.num_batches_tracked) == 5 and int(net.bn1d.num_batches_tracked) == 5
    assert {k: v.data_ptr() for k, v in net.named_buffers()} == ptrs       # reset in place
    assert net.bn2d.momentum == 0.3 and net.bn1d.momentum == 0.1
    assert not net.training and not net.bn2d.training and not net.conv.training and net.bn1d.training
    assert not any(p.grad is not None for p in net.parameters())


def test_reestimate_bn_takes_tuples_and_a_forward_callable():
    a, b, c = _net(), _net(), _net()
    assert reestimate_bn(a, _batches()) == 5
    assert reestimate_bn(b, [(x,) for x in _batches()]) == 5                # tuple or list: model(*batch)
    seen = []
    assert reestimate_bn(c, iter({"x": x} for x in _batches()), forward=lambda m, batch: seen.append(1) or m(batch["x"])) == 5
    assert len(seen) == 5
    for (k, v), (_, w), (_, u) in zip(a.named_buffers(), b.named_buffers(), c.named_buffers()):
        assert torch.equal(v, w) and torch.equal(v, u), k


def test_reestimate_bn_restores_momenta_and_flags_when_a_batch_raises():
    net = _net().eval()
    calls = []

    def forward(m, batch):
        calls.append(1)
        if len(calls) == 3:
            raise KeyError("third batch")
        return m(batch)

    with pytest.raises(KeyError):
        reestimate_bn(net, _batches(), forward)
    assert len(calls) == 3
    assert net.bn2d.momentum == 0.3 and net.bn1d.momentum == 0.1
    assert not any(m.training for m in net.modules())
    assert int(net.bn2d.num_batches_tracked) == 2          # two batches got through (update_bn's behaviour: the counters stay)


def test_reestimate_bn_with_no_batches_changes_nothing():
    net = _net().eval()
    before = {k: v.clone() for k, v in net.state_dict().items()}
    assert reestimate_bn(net, []) == 0
    assert reestimate_bn(net, iter(())) == 0
    assert all(torch.equal(v, before[k]) for k, v in net.state_dict().items())
    assert net.bn2d.momentum == 0.3 and not net.training


# ---- the argument checks of ema= ----------------------------------------------------------------------------------------------
class StubOpt:
    """what reestimate_bn reads of a FlatAdam: the buffers it averages, the swap state, the context manager"""

    def __init__(self, ebufs, swapped=False):
        self._ebufs, self._swapped, self.entered = list(ebufs), swapped, 0

    def _not_swapped(self, what):
        if self._swapped:
            raise RuntimeError(f"FlatAdam.{what} while the averaged weights are swapped in")

    @contextlib.contextmanager
    def ema_weights(self):
        self.entered += 1
        yield self


def _untouched(net, before):
    return all(torch.equal(v, before[k]) for k, v in net.state_dict().items()) and net.bn2d.momentum == 0.3 and not net.training


def test_reestimate_bn_with_ema_checks_its_arguments_before_anything_is_written():
    net = _net().eval()
    before = {k: v.clone() for k, v in net.state_dict().items()}
    stats = [(k, v) for k, v in net.named_buffers() if v.is_floating_point()]
    no_buffers = StubOpt([])
    with pytest.raises(ValueError, match="ema_buffers"):
        reestimate_bn(net, _batches(), ema=no_buffers)
    partial = StubOpt([kv for kv in stats if kv[0] != "bn1d.running_var"])
    with pytest.raises(ValueError, match="bn1d.running_var"):
        reestimate_bn(net, _batches(), ema=partial)
    copies = StubOpt([(k, v.clone()) for k, v in stats])   # the same names at other addresses: held by address
    with pytest.raises(ValueError, match="bn2d.running_mean"):
        reestimate_bn(net, _batches(), ema=copies)
    swapped = StubOpt(stats, swapped=True)
    with pytest.raises(RuntimeError, match="swapped in"):
        reestimate_bn(net, _batches(), ema=swapped)
    assert no_buffers.entered == partial.entered == copies.entered == swapped.entered == 0
    assert _untouched(net, before)


def test_reestimate_bn_with_ema_runs_inside_the_swap_and_puts_the_counters_back():
    net = _net().eval()
    counters = {k: v.clone() for k, v in net.named_buffers() if not v.is_floating_point()}
    ref = copy.deepcopy(net)
    reestimate_bn(ref, _batches())
    opt = StubOpt([(k, v) for k, v in net.named_buffers() if v.is_floating_point()])
    assert reestimate_bn(net, _batches(), ema=opt) == 5 and opt.entered == 1
    for (k, v), (_, r) in zip(net.named_buffers(), ref.named_buffers()):
        if v.is_floating_point():
            assert torch.equal(v, r), k                    # (the stub swaps nothing: the re-estimated statistics are in the model)
        else:
            assert torch.equal(v, counters[k]) and int(r) == 5, k
    untracked = torch.nn.Sequential(torch.nn.Conv2d(3, 5, 3), torch.nn.BatchNorm2d(5, track_running_stats=False))
    assert reestimate_bn(untracked, _batches(), ema=opt) == 5             # a BatchNorm without statistics has nothing to hold
