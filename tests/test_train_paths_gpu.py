"""The training step on the kernel families the default hparams never select (tests/train_cases.py: PATH_CASES): the staged
local-condition route, the other output heads and loss kernels, the front at other widths, the one-hot model away from Q = 256 -- each
against the float64 torch restatement under the bars of tests/test_train_gpu.py; and the optimiser kernels through the C-ABI directly.
Parity with a torch restatement of the reference graph, unpinned against TensorFlow like the rest of the training tests."""
import ctypes as C

import numpy as np
import pytest
import torch

import torch_train_ref as R
import train_cases as TC
from train_cases import _assert_against_float64

pytestmark = pytest.mark.gpu


def _on_route(tr, want):
    route = tr.route()
    assert {k: route[k] for k in want} == want, route


def _checkers(tensors, cfg, audio, lc, gc, q):
    l64, g64 = R.loss_and_grads(tensors, cfg, audio, lc, gc, quantized=q, dtype=torch.float64)
    l32, g32 = R.loss_and_grads(tensors, cfg, audio, lc, gc, quantized=q, dtype=torch.float32)
    return l64, g64, l32, g32


@pytest.mark.parametrize("cid", TC.PATH_IDS)
def test_loss_and_gradients_on_the_other_routes(cid):
    _, kw, want = TC.PATH_BY_ID[cid]
    tr, tensors, cfg, audio, lc, gc, q = TC._case6(**kw)
    _on_route(tr, want)                                                   # first: the case runs the kernels it is here for
    if q is not None:                                                     # the checker's class ids are the device quantizer's
        from twvk_amd.ops import mu_law_encode
        assert np.array_equal(mu_law_encode(torch.from_numpy(audio).cuda(), kw["Q"]).cpu().numpy(), q)
    loss = float(tr.loss_and_gradients(audio, lc, gc).item())
    got = tr.gradients()
    l64, g64, l32, g32 = _checkers(tensors, cfg, audio, lc, gc, q)
    _assert_against_float64(cid, loss, got, l64, g64, l32, g32)
    # the last layer's dense 1x1 has no path to the loss (its output feeds a layer that does not exist): exactly zero, not small
    last = "wavenet/dilated_stack/layer%d/dilation_layer/dense/" % (len(kw["dil"]) - 1)
    for k in [last + "kernel"] + ([last + "bias"] if kw.get("use_bias", True) else []):
        assert not g64[k].any(), k
        assert (got[k] == 0).all(), (cid, k, float(np.abs(got[k]).max()))
    if cid == "g64-card5":
        emb64, emb = g64["wavenet/gc_embedding"], got["wavenet/gc_embedding"]
        used = sorted(set(kw["gc_ids"]))
        assert used == [0, 1, 3]
        for i in range(kw["gc_card"]):
            if i in used:
                assert np.abs(emb64[i]).max() > 0
            else:
                assert not emb64[i].any() and (emb[i] == 0).all(), i      # ids 2 and 4: no batch entry, exactly zero
        # (rows 0, 1, 3 are the sums over 2, 2 and 3 batch entries: held to the checker by _assert_against_float64 above -- a scatter
        # that kept one entry per id would be off by a factor, far outside the bar)
        scale = float(np.abs(emb64).max())
        assert float(np.abs(emb[used] - emb64[used]).max()) <= max(TC.RATIO * float(np.abs(g32["wavenet/gc_embedding"] - emb64).max()), TC.FLOOR * scale)
    if cid == "clamp":
        b = got["wavenet/conv1d_2/bias"]
        assert (b[20:25] == 0).all() and np.abs(b[25:30]).min() > 0      # clamped log-scales: zero gradient (mixture.py:47 tf.maximum)


def test_staged_route_is_reproducible_and_a_second_step_equals_a_fresh_trainer():
    """the staged twin of part (2) of test_second_step_with_other_data_and_the_workspace_contract.  The staged kernels walk every tile
    (t_lo = 0), so nothing rests on rows that are never written again and no NaN filling is asked for."""
    kw = dict(dil=[1, 2, 4, 8, 1, 2], B=3, Tm=4, up=(15, 20), seed=4)
    trA, tensors, cfg, audio, lc, gc, _ = TC._case6(**kw)
    _on_route(trA, dict(lc="staged"))
    rng = np.random.RandomState(99)
    audio2 = ((rng.rand(*audio.shape) - 0.5) * 1.2).astype(np.float32)
    lc2 = (rng.randn(*lc.shape) * 0.7).astype(np.float32)
    gc2 = (1 - gc).astype(np.int32)
    lossA1 = float(trA.loss_and_gradients(audio, lc, gc).item()); gA1 = trA.grads.clone()
    trB = TC._case6(**kw)[0]
    lossB1 = float(trB.loss_and_gradients(audio, lc, gc).item())
    assert lossA1 == lossB1 and torch.equal(gA1, trB.grads), "two fresh trainers, same data: different bits"
    lossA2 = float(trA.loss_and_gradients(audio2, lc2, gc2).item()); gA2 = trA.grads.clone()       # second step, other data
    trC = TC._case6(**kw)[0]
    lossC = float(trC.loss_and_gradients(audio2, lc2, gc2).item())
    assert lossA2 == lossC and torch.equal(gA2, trC.grads), "a second step differs from a fresh trainer's first"
    assert lossA2 != lossA1
    l64, g64, l32, g32 = _checkers(tensors, cfg, audio2, lc2, gc2, None)
    _assert_against_float64("staged second step", lossA2, trA.gradients(), l64, g64, l32, g32)


@pytest.mark.parametrize("cid", ["two-stage", "onehot-staged"])
def test_a_few_optimiser_steps_on_the_staged_route(cid):
    _, kw, want = TC.PATH_BY_ID[cid]
    tr, tensors, cfg, audio, lc, gc, q = TC._case6(**kw)
    _on_route(tr, want)
    l0 = float(tr.step(audio, lc, gc).item())
    for _ in range(20):
        l1 = float(tr.step(audio, lc, gc).item())
    assert np.isfinite([l0, l1]).all() and l1 < l0, (l0, l1)


# ---- the optimiser kernels through the C-ABI -------------------------------------------------------------------------------------
def _abi():
    import twvk_amd  # noqa: F401
    from twvk_amd import _lib
    from twvk_amd.wavenet import _ptr, _stream
    return _lib, _lib.lib(), _ptr, _stream


@pytest.mark.parametrize("t", [1, 1000, 1000000])
@pytest.mark.parametrize("n", [1, 255, 257, 1000003, 9000001])        # 9 000 001 > 32 768 blocks x 256 threads: the grid-stride loop
def test_adam_ema_step_direct(n, t):
    _lib, L, _ptr, _stream = _abi()
    rng = np.random.RandomState(n % 1000 + t % 7)
    p0 = (rng.randn(n) * 0.05); g0 = rng.randn(n) * 0.3
    m0 = rng.randn(n) * 0.01; v0 = (rng.randn(n) * 0.01) ** 2 + 1e-4; e0 = p0 + rng.randn(n) * 1e-3
    lr, scale = 1e-3, 0.125
    dev = [torch.from_numpy(a.astype(np.float32)).cuda() for a in (p0, g0, m0, v0, e0)]
    host = [a.cpu().numpy().astype(np.float64) for a in dev]                       # the float32 values the kernel starts from
    g_before = dev[1].clone()
    _lib.check(L.twv_adam_ema_step(_ptr(dev[0]), _ptr(dev[1]), _ptr(dev[2]), _ptr(dev[3]), _ptr(dev[4]), n, lr, 0.9, 0.999, 1e-8, t, 0.9999, scale,
                                   _stream()))
    torch.cuda.synchronize()
    p, m, v, ema = R.adam_ema(host[0], host[1] * scale, host[2], host[3], host[4], t, lr)
    assert torch.equal(dev[1], g_before)                                           # the gradients are an input
    # tolerances of test_adam_and_ema_update_match_tf_formulas, for its reasons: one fp32 update of O(lr) -> 1e-6 absolute; m, v fp32
    # accumulators with cancellation -> atol scaled to max|.|; (1 - beta2) formed in float32 -> 5e-5 relative on v
    np.testing.assert_allclose(dev[0].cpu().numpy(), p, rtol=0, atol=1e-6)
    np.testing.assert_allclose(dev[4].cpu().numpy(), ema, rtol=0, atol=1e-6)
    np.testing.assert_allclose(dev[2].cpu().numpy(), m, rtol=1e-5, atol=1e-6 * np.abs(m).max())
    np.testing.assert_allclose(dev[3].cpu().numpy(), v, rtol=5e-5, atol=1e-6 * np.abs(v).max())
    assert np.abs(dev[0].cpu().numpy() - host[0]).max() > 0                       # (it did move)


def test_adam_ema_step_edges():
    _lib, L, _ptr, _stream = _abi()
    bufs = [torch.full((64,), float(i + 1), device="cuda") for i in range(5)]
    keep = [b.clone() for b in bufs]
    _lib.check(L.twv_adam_ema_step(*[_ptr(b) for b in bufs], 0, 1e-3, 0.9, 0.999, 1e-8, 1, 0.9999, 1.0, _stream()))      # n = 0: OK, nothing written
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(bufs, keep))
    rc = L.twv_adam_ema_step(*[_ptr(b) for b in bufs], 64, 1e-3, 0.9, 0.999, 1e-8, 0, 0.9999, 1.0, _stream())            # t = 0: no such update
    assert rc == 1                                                                 # TWV_E_INVALID (include/twv_amd.h)
    with pytest.raises(_lib.TwvError):
        _lib.check(rc)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(bufs, keep))


@pytest.mark.parametrize("above", [True, False], ids=["above-the-clip", "below-the-clip"])
@pytest.mark.parametrize("n", [1, 1023, 1025, 1000003])
def test_clip_by_global_norm_direct(n, above):
    """grads <- g * pre * clip / max(||g * pre||, clip); the scratch is n + 1024 floats and nothing behind it is written"""
    _lib, L, _ptr, _stream = _abi()
    rng = np.random.RandomState(n % 1000)
    pre, clip = 0.25, 1.0
    g = rng.randn(n).astype(np.float32)
    nrm = np.sqrt(((g.astype(np.float64) * pre) ** 2).sum())
    g = (g * np.float32((3.0 if above else 0.4) / nrm)).astype(np.float32)         # scaled norm 3 or 0.4 against a clip of 1
    g64 = g.astype(np.float64) * pre
    nrm = np.sqrt((g64 ** 2).sum())
    assert (nrm > clip) == above
    want = g64 * clip / max(nrm, clip)
    GUARD, MARK = 4096, -12345.5
    scratch = torch.full((n + 1024 + GUARD,), MARK, dtype=torch.float32, device="cuda")
    dg = torch.from_numpy(g).cuda()
    _lib.check(L.twv_clip_by_global_norm(_ptr(dg), n, pre, clip, _ptr(scratch), _stream()))
    torch.cuda.synchronize()
    got = dg.cpu().numpy()
    np.testing.assert_allclose(got, want, rtol=1e-5, atol=0)                       # the bar the existing clipping test holds the norm to
    if not above:
        np.testing.assert_allclose(got, g64, rtol=1e-6, atol=0)                    # below the clip: g * pre_scale and nothing else
    s = scratch.cpu().numpy()
    assert (s[n + 1024:] == MARK).all(), "twv_clip_by_global_norm wrote behind the n + 1024 floats it is given"
    # the layout the header promises room for: n squares (rounded up to 64), 256 partial sums at most, the sum at partials + 512
    part = (n + 63) // 64 * 64
    assert part + 512 < n + 1024
    np.testing.assert_allclose(s[:n], g64 ** 2, rtol=1e-6, atol=0)
    np.testing.assert_allclose(s[part + 512], nrm ** 2, rtol=1e-5)                 # the last element written in the partial-sum region
    assert (s[part + 513:n + 1024] == MARK).all()
