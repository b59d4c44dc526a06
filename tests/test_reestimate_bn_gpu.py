"""BatchNorm re-estimation on an adapter site (avmoe_amd.train.reestimate_bn; BatchNorm momentum=None reaches the site kernels as
avmoe_moe_desc.bn_momentum < 0): torch.optim.swa_utils.update_bn drives a model that contains a site, reestimate_bn equals it bit for
bit, and with `ema=opt` the re-estimated statistics land in FlatAdam's shadows while the model's raw weights, raw statistics and
counters stay what they were.  The model and helpers are those of tests/test_flat_adam_ema_gpu.py."""
import copy

import pytest
import torch

from tests.test_flat_adam_ema_gpu import DECAY, LR, WD, OneSite, bits

pytestmark = pytest.mark.gpu

N_BATCHES = 4


def _model(seed, dev):
    torch.manual_seed(seed)
    model = OneSite()
    with torch.no_grad():                                    # the reference's zero gates make the output 0 whatever the statistics are
        for k, p in model.named_parameters():
            if k.endswith(("gate", "gate_av")):
                p.fill_(0.4)
    return model.to(dev).train()


def _batches(dev, n=N_BATCHES, seed=21):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(4, 64, 50, 1, generator=g).to(dev), torch.randn(4, 48, 20, 1, generator=g).to(dev)) for _ in range(n)]


def _site_forward(model, batch):
    return model.audio_adapter_blocks_p1[0](*batch)


def _bns(model):
    return [m for m in model.modules() if isinstance(m, torch.nn.modules.batchnorm._BatchNorm)]


class FixedY(torch.nn.Module):
    """what update_bn can drive: forward(x) with the other modality fixed"""

    def __init__(self, model, Y):
        super().__init__()
        self.model, self.Y = model, Y

    def forward(self, x):
        return self.model.audio_adapter_blocks_p1[0](x, self.Y)


def test_torch_update_bn_drives_a_model_with_a_site_and_reestimate_bn_equals_it():
    from avmoe_amd.train import reestimate_bn
    dev = torch.device("cuda:0")
    batches = _batches(dev)
    a = FixedY(_model(0, dev), batches[0][1])
    with torch.no_grad():                                    # statistics and counters away from their reset values
        a(batches[1][0])
    a.eval()
    b = copy.deepcopy(a)
    xs = [x for x, _y in batches]
    torch.optim.swa_utils.update_bn(xs, a)
    assert reestimate_bn(b, xs) == N_BATCHES
    n = 0
    for (k, v), (_, w) in zip(a.named_buffers(), b.named_buffers()):
        assert torch.equal(v, w) and (not v.is_floating_point() or torch.equal(bits(v), bits(w))), k
        if k.endswith("num_batches_tracked"):
            assert int(v) == N_BATCHES, k
            n += 1
        else:
            assert torch.isfinite(v).all(), k
    assert n == len(_bns(a)) == 8
    assert all(m.momentum == 0.1 for m in _bns(a) + _bns(b)) and not a.training and not b.training
    means = [v for k, v in b.named_buffers() if k.endswith("running_mean")]
    assert any(float(v.abs().max()) > 0 for v in means)      # re-estimated, not merely reset


def _trained(dev):
    from avmoe_amd.dp import AdapterGradReducer
    from avmoe_amd.train import FlatAdam
    model = _model(0, dev)
    site = model.audio_adapter_blocks_p1[0]
    red = AdapterGradReducer(list(site.parameters()), sites=[site])
    opt = FlatAdam(red, lr=LR, weight_decay=WD, max_grad_norm=1.0, ema_decay=DECAY, ema_warmup=1.0, ema_buffers=model)
    g = torch.Generator().manual_seed(9)
    for _ in range(6):
        X, Y = torch.randn(4, 64, 50, 1, generator=g).to(dev), torch.randn(4, 48, 20, 1, generator=g).to(dev)
        G = torch.randn(4, 64, 50, 1, generator=g).to(dev)
        red.begin(sync=True)
        site(X, Y)[0].backward(G)
        red.finish()
        opt.step()
        red.zero_grad()
    return model, site, opt


def test_reestimate_bn_under_the_averaged_weights_writes_the_shadows_and_leaves_the_model_alone():
    from avmoe_amd.train import adapter_state_dict, load_adapters, reestimate_bn
    dev = torch.device("cuda:0")
    model, site, opt = _trained(dev)
    batches = _batches(dev)
    sd_avg = adapter_state_dict(model, ema=opt)              # the averaged model, before the call
    raw = {k: v.detach().clone() for k, v in model.state_dict().items()}
    ptrs = {k: v.data_ptr() for k, v in model.named_buffers()}
    flags = [m.training for m in model.modules()]
    shadows_before = [e.clone() for e in opt.ema_buffers]
    assert reestimate_bn(model, batches, _site_forward, ema=opt) == N_BATCHES
    for k, v in model.state_dict().items():                  # parameters, statistics, counters: bit for bit what they were
        assert torch.equal(v, raw[k]) and (v.dtype != torch.float32 or torch.equal(bits(v), bits(raw[k]))), k
        if k.endswith("num_batches_tracked"):
            assert int(v) == 6, k
    assert {k: v.data_ptr() for k, v in model.named_buffers()} == ptrs
    assert all(m.momentum == 0.1 for m in _bns(model)) and [m.training for m in model.modules()] == flags
    assert not opt._swapped
    torch.manual_seed(1)
    fresh = OneSite()
    res = load_adapters(fresh, sd_avg)
    assert not res.unexpected_keys and not [k for k in res.missing_keys if "adapter" in k]
    fresh = fresh.to(dev)
    assert reestimate_bn(fresh, batches, _site_forward) == N_BATCHES
    want = dict(fresh.named_buffers())
    changed = 0
    for k, e, old in zip(opt.ema_buffer_names, opt.ema_buffers, shadows_before):
        assert torch.equal(bits(e), bits(want[k])), k        # the shadows are the statistics of the averaged weights on these batches
        changed += not torch.equal(e, old)
    assert changed == len(opt.ema_buffer_names) > 0          # and not what averaging had left there
    model.eval(); fresh.eval()
    with torch.no_grad():
        with opt.ema_weights():
            out_avg = _site_forward(model, batches[0])[0].clone()
        out_fresh = _site_forward(fresh, batches[0])[0]
    assert torch.equal(bits(out_avg), bits(out_fresh)) and float(out_avg.abs().max()) > 0


def test_a_batch_that_raises_leaves_the_model_swapped_back_with_momenta_and_counters_restored():
    from avmoe_amd.train import reestimate_bn
    dev = torch.device("cuda:0")
    model, site, opt = _trained(dev)
    raw = {k: v.detach().clone() for k, v in model.state_dict().items()}
    calls = []

    def forward(m, batch):
        calls.append(1)
        if len(calls) == 2:
            raise KeyError("second batch")
        return _site_forward(m, batch)

    with pytest.raises(KeyError):
        reestimate_bn(model, _batches(dev), forward, ema=opt)
    assert len(calls) == 2 and not opt._swapped
    assert all(m.momentum == 0.1 for m in _bns(model)) and model.training
    for k, v in model.state_dict().items():
        assert torch.equal(v, raw[k]), k
