"""BN statistics re-estimation, the parts that need no GPU (fp8_quantization_amd.bn_reestimate).

  * the host logic on stub modules -- plain nn.Modules with the BN-fused layers' duck type whose
    forward leaves known per-batch statistics in running_*: the sums, the division, the momentum
    restore, training mode on the layer alone, store_ema_stats, num_batches < 1;
  * gloo world size 2: rank r runs batches r::2, one packed all-reduce, both ranks end with identical
    bytes, equal to the world-1 result over the same four batches (the hand-filled values are exact in
    fp32, sums included, so the comparison is bitwise);
  * the driver's flags and the C-ABI's host-only workspace query;
  * the reference fixture tests/golden/bn_reestimate.npz (the reference's own reestimate_BN_stats on
    its QuantizedMobileNetV2, tests/golden/gen_golden_bnre.py): final statistics = the fp32 mean of the
    recorded per-batch ones, and torch's fp32 batch statistics against float64 ones of the recorded
    pre-BN tensors.  Bars (u = 2^-24, n values per channel, A = max |x| of the channel): an fp32
    sum of n terms in ANY order errs by at most (n - 1) u sum |x| (1 + O(n u)), so the mean by
    n u A; the variance, a mean of n squares of deviations each within 2 |d| (n u A) + 3 u d^2 of the
    exact one, by (n + 4) u Dm^2 + 2 Dm n u A with Dm = max |x - mean|.  This fixes how far the
    reference itself may sit from float64; the GPU test adds the recorded distance to its own bar.
"""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
from torch import nn

from tests import golden_io as gio

U = 2.0 ** -24


class StubBN(nn.Module):
    """The duck type (running_mean, running_var, gamma, momentum, run_forward) and a forward that
    leaves batch i's statistics -- i is the input's first value -- in the running buffers."""

    def __init__(self, C, scale):
        super().__init__()
        self.register_buffer("running_mean", torch.full((C,), -1.0))
        self.register_buffer("running_var", torch.full((C,), 9.0))
        self.gamma = nn.Parameter(torch.ones(C))
        self.momentum = 0.25
        self.child = nn.Dropout(0.5)
        self.scale = scale
        self.seen = []

    def run_forward(self, x, weight, bias, offsets=None):
        raise NotImplementedError

    def stats(self, i):
        C = self.running_mean.numel()
        base = torch.arange(C, dtype=torch.float32)
        return self.scale * (base + i), self.scale * (base * 0.5 + 2.0 * i + 1.0)  # exact in fp32

    def forward(self, x):
        assert self.training and self.momentum == 1.0 and not self.child.training
        i = int(x.reshape(-1)[0])
        self.seen.append(i)
        m, v = self.stats(i)
        self.running_mean.copy_(m)
        self.running_var.copy_(v)
        return x


class BNFusedHijacker(StubBN):
    """A foreign class of the reference's name: recognised by its duck type, not by isinstance."""


def stub_model():
    return nn.Sequential(StubBN(3, 1.0), nn.ReLU(), BNFusedHijacker(5, 0.25), nn.Linear(1, 1))


def batches(n):
    return [(torch.full((1, 1), float(i)), i) for i in range(n)]


def expected(mod, ids):
    ms, vs = zip(*(mod.stats(i) for i in ids))
    return sum(ms) / len(ids), sum(vs) / len(ids)


def test_stub_sums_division_and_restore():
    from fp8_quantization_amd.bn_reestimate import bn_fused_layers, reestimate_bn_stats
    model = stub_model().train()
    assert [n for n, _ in bn_fused_layers(model)] == ["0", "2"]
    ptr = model[0].running_mean.data_ptr()
    v0 = model[0].running_mean._version
    n = reestimate_bn_stats(model, batches(6), num_batches=4)
    assert n == 4
    for mod in (model[0], model[2]):
        assert mod.seen == [0, 1, 2, 3]
        m, v = expected(mod, range(4))
        assert torch.equal(mod.running_mean, m) and torch.equal(mod.running_var, v)
        assert torch.equal(mod.running_mean_sum, m * 4) and torch.equal(mod.running_var_sum, v * 4)
        assert mod.momentum == 0.25 and not mod.training and not mod.child.training
        assert not hasattr(mod, "running_mean_ema")
    assert not model.training
    # in place: the same storage, a newer version (what the eval store's cache keys on)
    assert model[0].running_mean.data_ptr() == ptr and model[0].running_mean._version > v0
    # a loader shorter than num_batches: the mean over what it held
    model = stub_model()
    assert reestimate_bn_stats(model, batches(3), num_batches=50) == 3
    assert torch.equal(model[2].running_mean, expected(model[2], range(3))[0])


def test_class_tuple_instead_of_duck_type():
    """With a class (tuple) only its instances are re-estimated: the other duck-typed layer stays in
    eval mode and keeps its buffers."""
    from fp8_quantization_amd.bn_reestimate import reestimate_bn_stats

    class Plain(StubBN):
        def forward(self, x):
            assert not self.training
            return x
    model = nn.Sequential(Plain(2, 1.0), BNFusedHijacker(2, 1.0))
    reestimate_bn_stats(model, batches(2), num_batches=2, classes=(BNFusedHijacker,))
    assert torch.equal(model[0].running_var, torch.full((2,), 9.0)) and model[0].momentum == 0.25
    assert torch.equal(model[1].running_var, expected(model[1], range(2))[1])


def test_store_ema_stats():
    from fp8_quantization_amd.bn_reestimate import reestimate_bn_stats
    model = stub_model()
    reestimate_bn_stats(model, batches(2), num_batches=2, store_ema_stats=True)
    mod = model[0]
    assert "running_mean_ema" in dict(mod.named_buffers()) and "running_var_ema" in mod.state_dict()
    assert torch.equal(mod.running_mean_ema, torch.full((3,), -1.0)) and torch.equal(mod.running_var_ema,
                                                                                      torch.full((3,), 9.0))
    first = mod.running_mean.clone()
    reestimate_bn_stats(model, batches(4)[2:], num_batches=2, store_ema_stats=True)  # refreshed, still a buffer
    assert torch.equal(mod.running_mean_ema, first) and "running_mean_ema" in dict(mod.named_buffers())
    assert torch.equal(mod.running_mean, expected(mod, [2, 3])[0])


@pytest.mark.parametrize("n", [0, -1])
def test_num_batches_below_one_raises(n):
    from fp8_quantization_amd.bn_reestimate import reestimate_bn_stats
    model = stub_model()
    with pytest.raises(ValueError):
        reestimate_bn_stats(model, batches(2), num_batches=n)
    assert model[0].seen == [] and model[0].momentum == 0.25


# ------------------------------------------------------------------------------------ gloo, world 2
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, ws, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=ws)
    try:
        from fp8_quantization_amd.bn_reestimate import reestimate_bn_stats
        model = stub_model()
        n = reestimate_bn_stats(model, batches(6), num_batches=4)
        q.put((rank, n, [m.seen for m in (model[0], model[2])],
               [t.numpy().tobytes() for m in (model[0], model[2]) for t in (m.running_mean, m.running_var)]))
    finally:
        dist.destroy_process_group()


def test_gloo_world2_packed_allreduce():
    from fp8_quantization_amd.bn_reestimate import reestimate_bn_stats
    ws = 2
    port = _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, ws, port, q)) for r in range(ws)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=120) for _ in range(ws)], key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert res[0][2] == [[0, 2], [0, 2]] and res[1][2] == [[1, 3], [1, 3]]  # rank r: batches r::2 of the first 4
    assert res[0][1] == res[1][1] == 4
    assert res[0][3] == res[1][3]  # identical bytes on both ranks
    single = stub_model()
    reestimate_bn_stats(single, batches(6), num_batches=4)
    want = [t.numpy().tobytes() for m in (single[0], single[2]) for t in (m.running_mean, m.running_var)]
    assert res[0][3] == want  # (exact fp32 values: no summation-order slack to grant)


# ------------------------------------------------------------------------------------ driver, ABI
def test_driver_flags():
    from fp8_quantization_amd import imagenet
    a = imagenet.parse([])
    assert a.reestimate_bn_stats is False and a.bn_batches is None
    # the defaults every earlier run relied on
    assert (a.arch, a.image_size, a.batch_size, a.num_workers, a.num_est_batches, a.mini_test, a.max_batches) == \
        ("resnet18", 224, 16, 8, 1, False, 0)
    assert (a.expo_width, a.mant_width, a.dnsmp_factor, a.with_comp, a.no_approx, a.no_s2n, a.no_qbma) == \
        (4, 3, 3, False, False, False, False)
    assert (a.weight_quant_method, a.act_quant_method, a.synthetic, a.images_dir, a.weights, a.output) == \
        ("current_minmax", "allminmax", 0, None, None, None)
    b = imagenet.parse(["--reestimate-bn-stats", "--bn-batches", "7"])
    assert b.reestimate_bn_stats is True and b.bn_batches == 7
    assert imagenet.parse(["--no-reestimate-bn-stats"]).reestimate_bn_stats is False
    # --synthetic sizes its train set for max(num_est_batches, bn_batches) batches
    c = imagenet.parse(["--synthetic", "8", "--batch-size", "4", "--reestimate-bn-stats", "--bn-batches", "3"])
    assert len(imagenet.datasets(c)[1]) == 12 and imagenet.bn_batch_count(c, imagenet.datasets(c)[1]) == 3
    d = imagenet.parse(["--synthetic", "8", "--batch-size", "4", "--bn-batches", "3"])
    assert len(imagenet.datasets(d)[1]) == 4  # flag off: as before
    # the reference's default: int(0.002 * number of train batches)
    e = imagenet.parse(["--batch-size", "16", "--reestimate-bn-stats"])
    assert imagenet.bn_batch_count(e, range(1281167)) == int(0.002 * 80073) == 160


def test_bn_train_workspace_query_is_host_only():
    from fp8_quantization_amd import _lib
    L = _lib.load()
    assert {"fp8a_bn_train", "fp8a_bn_train_workspace_size"} <= set(_lib.SYMBOLS)
    a, b = L.fp8a_bn_train_workspace_size(4, 8, 49), L.fp8a_bn_train_workspace_size(4, 64, 49)
    assert 0 < a < b and b == 8 * a  # one (S, Q) double pair per (channel, part): grows with C
    assert L.fp8a_bn_train_workspace_size(16, 4096, 1) >= 4096 * 16
    assert L.fp8a_bn_train_workspace_size(0, 8, 49) == 0 and L.fp8a_bn_train_workspace_size(4, 0, 49) == 0
    # n == 1 -> the code check() maps to ValueError, before any launch or pointer is looked at
    rc = L.fp8a_bn_train(None, None, 1, 3, 1, None, None, 1e-5, 0.1, None, None, None, None, None, 0, 0.0, 0.0, None,
                         0, 0, 0, None, None, None, 0, None)
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        _lib.check(rc, "fp8a_bn_train")
    rc = L.fp8a_bn_train(None, None, 0, 3, 1, None, None, 1e-5, 0.1, None, None, None, None, None, 0, 0.0, 0.0, None,
                         0, 0, 0, None, None, None, 0, None)
    with pytest.raises(AssertionError):
        _lib.check(rc, "fp8a_bn_train")


# ------------------------------------------------------------------------------------ the fixture
def ref_distance(g, layer, b):
    """(|mean - mean64|, |biased var - var64|) of the reference's recorded fp32 statistics of batch b."""
    pre = g[f"pre{b}/{layer}"]
    n = pre.size // pre.shape[1]
    mean = g[f"stat_mean{b}/{layer}"].astype(np.float64)
    var = g[f"stat_var{b}/{layer}"].astype(np.float64) * (n - 1) / n  # the buffers hold the unbiased one
    return np.abs(mean - g[f"mean64{b}/{layer}"]), np.abs(var - g[f"var64{b}/{layer}"]), n


def test_reference_fixture_is_consistent():
    g = gio.load("bn_reestimate.npz")
    layers, teacher = [str(s) for s in g["layers"]], [str(s) for s in g["teacher"]]
    assert len(layers) == 52 and len(teacher) == 3 and set(teacher) <= set(layers)
    assert g["x0"].shape == g["x1"].shape == (4, 3, 32, 32)
    for name in layers:
        assert g[f"final_mean/{name}"].shape == g[f"init_mean/{name}"].shape
        assert np.isfinite(g[f"final_mean/{name}"]).all() and (g[f"final_var/{name}"] >= 0).all()
    for name in teacher:
        # final = (0 + batch 0 + batch 1) / 2 in fp32, as qat_utils.py:91-104 forms it
        for key in ("mean", "var"):
            s = (g[f"stat_{key}0/{name}"] + g[f"stat_{key}1/{name}"]) / np.float32(2)
            assert np.array_equal(s, g[f"final_{key}/{name}"]), (name, key)
        for b in (0, 1):
            pre = g[f"pre{b}/{name}"].astype(np.float64)
            C = pre.shape[1]
            x = np.moveaxis(pre, 1, 0).reshape(C, -1)
            assert np.allclose(x.mean(1), g[f"mean64{b}/{name}"], rtol=0, atol=1e-12 * np.abs(x).max())
            em, ev, n = ref_distance(g, name, b)
            A = np.abs(x).max(1)
            Dm = np.abs(x - g[f"mean64{b}/{name}"][:, None]).max(1)
            assert (em <= n * U * A + 1e-45).all(), (name, b, (em / (n * U * A + 1e-45)).max())
            bar_v = (n + 4) * U * Dm ** 2 + 2 * Dm * n * U * A + 1e-45
            assert (ev <= bar_v).all(), (name, b, (ev / bar_v).max())
