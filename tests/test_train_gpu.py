"""C4: the teacher-forced WaveNet training step on the MI355X vs a plain PyTorch fp32 (CPU autograd) model of the same op.

Floating-point work -> tolerance parity (written at each assert).  The GPU path sums in a different order (rocBLAS
GEMMs over all rows, chunked column sums), so agreement is to fp32 round-off of the reductions, not bit-exact."""
import os

import numpy as np
import pytest
import torch

import torch_train_ref as R
from helpers import make_model
from train_cases import DEFAULT_CASES, FLOOR, LOSS_FLOOR, RATIO, UP, _assert_against_float64, _case      # noqa: F401

pytestmark = pytest.mark.gpu

# (the case builder, the bars RATIO = 8, FLOOR = 5e-6, LOSS_FLOOR = 2e-6 and the data they come from: tests/train_cases.py)
assert (RATIO, FLOOR, LOSS_FLOOR) == (8.0, 5e-6, 2e-6)


def _check_grads(got, ref, rtol):
    """the older form (one float32 reference, a flat tolerance relative to each tensor's largest element): only for the L2 / clipping
    options case below, whose sigma = 0.3 weights saturate the gates"""
    for name, r in ref.items():
        g = got[name]
        scale = max(float(np.abs(r).max()), 1e-12)
        err = float(np.abs(g - r).max()) / scale
        assert np.isfinite(g).all(), name
        assert err <= rtol, "%s: max|diff| = %.3g of max|ref| %.3g" % (name, err, scale)


@pytest.mark.parametrize("kw", [kw for _, kw in DEFAULT_CASES], ids=[i for i, _ in DEFAULT_CASES])
def test_loss_and_gradients_match_torch_fp32(kw, request):
    tr, tensors, cfg, audio, lc, gc = _case(**kw)
    loss = float(tr.loss_and_gradients(audio, lc, gc).item())
    l64, g64 = R.loss_and_grads(tensors, cfg, audio, lc, gc, dtype=torch.float64)
    l32, g32 = R.loss_and_grads(tensors, cfg, audio, lc, gc, dtype=torch.float32)
    _assert_against_float64(request.node.callspec.id, loss, tr.gradients(), l64, g64, l32, g32)


def test_loss_and_gradients_at_bench_geometry():
    """BASELINE configs[3]'s own geometry in the small: 30 layers (3x[1..512], receptive field 3101), S = 512 and a batch of
    16 x 3600 samples, which takes the 16-slab split-K path of the wide weight gradients that bench.py's B = 64 takes.  Through 30
    layers some gradients (lc kernels of the early layers) are ~1e-9 of the largest and sit at fp32 round-off of a 57 600-row
    reduction (the float32 torch model is 4e-3 of the tensor's max away from float64 there), so the bar is stated against float64,
    relative to the float32 torch model's own distance (RATIO / FLOOR above)."""
    tr, tensors, cfg, audio, lc, gc = _case(dil=[2 ** i for i in range(10)] * 3, B=16, Tm=12, S=512)
    loss = float(tr.loss_and_gradients(audio, lc, gc).item())
    got = tr.gradients()
    l64, g64 = R.loss_and_grads(tensors, cfg, audio, lc, gc, dtype=torch.float64)
    l32, g32 = R.loss_and_grads(tensors, cfg, audio, lc, gc, dtype=torch.float32)
    _assert_against_float64("16 x 3600", loss, got, l64, g64, l32, g32)


def test_one_step_at_the_full_configs3_batch():
    """BASELINE configs[3] at its own size: ONE teacher-forced step of B = 64 crops x 7800 samples (8000 floored to a hop multiple,
    datafeeder_wavenet.py:41-47), 30 layers, S = 512, MoL loss -- the batch bench.py times.  The checker is the torch restatement
    in float64, run on the GPU in its matmul form (tests/torch_train_ref.py:network_mm; ~0.5 M rows per matmul); the float32
    torch model beside it gives the scale of plain round-off.  Same bars as every other geometry (RATIO / FLOOR / LOSS_FLOOR above)."""
    dil = [2 ** i for i in range(10)] * 3
    tr, tensors, cfg, audio, lc, gc = _case(dil=dil, B=64, Tm=26, S=512)
    assert audio.shape == (64, 7800)
    loss = float(tr.loss_and_gradients(audio, lc, gc).item())
    got = tr.gradients()
    l64, g64 = R.loss_and_grads(tensors, cfg, audio, lc, gc, dtype=torch.float64, device="cuda:0", matmul_form=True)
    torch.cuda.empty_cache()
    l32, g32 = R.loss_and_grads(tensors, cfg, audio, lc, gc, dtype=torch.float32, device="cuda:0", matmul_form=True)
    torch.cuda.empty_cache()
    sampled = ["wavenet/conv1d_2/kernel", "wavenet/dilated_stack/layer29/dilation_layer/skip/kernel",
               "wavenet/dilated_stack/layer0/dilation_layer/conv_filter/kernel", "wavenet/upsample0/kernel"]
    assert all(k in g64 for k in sampled)
    _assert_against_float64("64 x 7800", loss, got, l64, g64, l32, g32)


def test_gradients_against_float64_reference_are_closer_than_float32_noise():
    """the fp32 torch model itself deviates from float64 by round-off; the HIP path must be in the same league"""
    tr, tensors, cfg, audio, lc, gc = _case(dil=[1, 2, 4, 1, 2], B=2, Tm=3)
    tr.loss_and_gradients(audio, lc, gc)
    got = tr.gradients()
    _, g64 = R.loss_and_grads(tensors, cfg, audio, lc, gc, dtype=torch.float64)
    _, g32 = R.loss_and_grads(tensors, cfg, audio, lc, gc, dtype=torch.float32)
    e_hip = max(float(np.abs(got[k] - g64[k]).max()) / max(float(np.abs(g64[k]).max()), 1e-12) for k in g64)
    e_t32 = max(float(np.abs(g32[k] - g64[k]).max()) / max(float(np.abs(g64[k]).max()), 1e-12) for k in g64)
    assert e_hip <= max(20 * e_t32, 1e-4), (e_hip, e_t32)


def test_adam_and_ema_update_match_tf_formulas():
    tr, tensors, cfg, audio, lc, gc = _case(dil=[1, 2, 4, 1, 2], B=2, Tm=3)
    p = tr.params.cpu().numpy().astype(np.float64)
    m = np.zeros_like(p); v = np.zeros_like(p); ema = p.copy()
    for it in range(3):
        tr.loss_and_gradients(audio, lc, gc)
        g = tr.grads.cpu().numpy().astype(np.float64)
        lr = tr.apply_gradients()
        assert lr == pytest.approx(1e-3 * 0.5 ** (it / 300000.0), rel=1e-12)          # model.py:320
        p, m, v, ema = R.adam_ema(p, g, m, v, ema, it + 1, lr)
        # tolerance: one fp32 update of O(lr) on O(0.05) weights -> 1e-6 absolute
        np.testing.assert_allclose(tr.params.cpu().numpy(), p, rtol=0, atol=1e-6)
        np.testing.assert_allclose(tr.ema.cpu().numpy(), ema, rtol=0, atol=1e-6)
        # m, v: fp32 accumulators; elements where beta*m and (1-beta)*g cancel lose relative accuracy -> atol scaled to max|.|
        np.testing.assert_allclose(tr.m.cpu().numpy(), m, rtol=1e-5, atol=1e-6 * np.abs(m).max())
        # (1 - beta2) is formed in float32 as TF's kernel does: 1 - 0.999f carries a 1.3e-5 relative rounding
        np.testing.assert_allclose(tr.v.cpu().numpy(), v, rtol=5e-5, atol=1e-6 * np.abs(v).max())
        p = tr.params.cpu().numpy().astype(np.float64); m = tr.m.cpu().numpy().astype(np.float64)
        v = tr.v.cpu().numpy().astype(np.float64); ema = tr.ema.cpu().numpy().astype(np.float64)
    assert tr.global_step == 3


def test_training_reduces_the_loss_and_trained_weights_generate():
    """a few steps on one fixed batch: the loss must fall; the EMA weights load into the generation path"""
    tr, tensors, cfg, audio, lc, gc = _case(dil=[1, 2, 4, 8, 1, 2, 4, 8], B=4, Tm=4, S=64)
    losses = [float(tr.step(audio, lc, gc).item()) for _ in range(30)]
    assert np.isfinite(losses).all()
    assert losses[-1] < losses[0] - 0.5, losses
    gen = make_model(1, [1, 2, 4, 8, 1, 2, 4, 8], tr.ema_weights(), S=64)
    from helpers import mol_uniforms
    up = gen.create_upsample(torch.from_numpy(lc[:1]).cuda())
    out = gen.generate(up[:, :300].contiguous(), [int(gc[0])], np.zeros(1, np.float32), mol_uniforms(1, 300, 10))
    assert np.isfinite(out.cpu().numpy()).all()


def test_bad_shapes_are_rejected():
    tr, tensors, cfg, audio, lc, gc = _case(dil=[1, 2, 4], B=2, Tm=2)
    with pytest.raises(ValueError):
        tr.loss_and_gradients(audio[:, :-1], lc, gc)
    with pytest.raises(ValueError):
        tr.loss_and_gradients(audio, lc[:, :1], gc)
    from twvk_amd.train import WaveNetTrainer
    from twvk_amd._lib import TwvError
    with pytest.raises(TwvError):
        WaveNetTrainer(tr.net, sample_size=0)        # shorter than the receptive field


def test_onehot_mulaw_model_loss_and_gradients():
    """scalar_input=False: mu-law one-hot input, width-2 causal conv over Q channels, softmax cross-entropy (model.py:257-296)"""
    import twvk_amd  # noqa: F401
    from twvk_amd import weights as W
    from twvk_amd.ops import mu_law_encode
    from twvk_amd.train import WaveNetTrainer
    dil, B, Tm, S, Q = [1, 2, 4, 8, 1, 2], 2, 2, 64, 256
    specs = W.tensor_specs(len(dil), S=S, Q=Q, scalar_input=False)
    tensors = W.random_tensors(specs, seed=3, scale=0.1)
    T = Tm * 300
    rng = np.random.RandomState(4)
    audio = ((rng.rand(B, T) - 0.5) * 1.8).astype(np.float32)
    lc = (rng.randn(B, Tm, 80) * 0.5).astype(np.float32)
    gc = np.array([1, 0], np.int32)
    net = make_model(B, dil, tensors, S=S, Q=Q, scalar_input=False)
    tr = WaveNetTrainer(net, sample_size=T)
    tr.load_weights(tensors)
    loss = float(tr.loss_and_gradients(audio, lc, gc).item())
    q = mu_law_encode(torch.from_numpy(audio).cuda(), Q).cpu().numpy()      # the quantizer itself is pinned bit-exact elsewhere
    cfg = dict(dilations=dil, initial_filter_width=32, use_biases=True, upsample_factor=UP, scalar_input=False, Q=Q)
    l64, g64 = R.loss_and_grads(tensors, cfg, audio, lc, gc, quantized=q, dtype=torch.float64)
    l32, g32 = R.loss_and_grads(tensors, cfg, audio, lc, gc, quantized=q, dtype=torch.float32)
    _assert_against_float64("one-hot", loss, tr.gradients(), l64, g64, l32, g32)      # the same bars as the MoL model
    l0 = float(tr.step(audio, lc, gc).item())
    for _ in range(20):
        l1 = float(tr.step(audio, lc, gc).item())
    assert l1 < l0


def test_l2_and_gradient_clipping_options():
    """model.py:300-312 (L2 on non-bias variables) and model.py:330-331 (clip_by_global_norm(gradients, 1.))"""
    tr, tensors, cfg, audio, lc, gc = _case(dil=[1, 2, 4, 1, 2], B=2, Tm=3, scale=0.3)
    base_loss, base_g = R.loss_and_grads(tensors, cfg, audio, lc, gc)
    lam = 0.01
    tr.l2 = lam
    loss = float(tr.loss_and_gradients(audio, lc, gc).item())
    l2 = sum(0.5 * float((np.asarray(v, np.float64) ** 2).sum()) for k, v in tensors.items() if "bias" not in k)
    assert abs(loss - (base_loss + lam * l2)) <= 2e-5 * abs(base_loss + lam * l2)
    want = {k: base_g[k] + (0 if "bias" in k else lam * tensors[k]) for k in base_g}
    # tolerance 5e-3 of each tensor's max: this case uses sigma = 0.3 weights (saturating gates), where fp32 round-off of ANY
    # summation order is amplified through the stack (torch f32 vs f64 differ by ~1e-3 here)
    _check_grads(tr.gradients(), want, 5e-3)
    # clipping: the flat gradient is rescaled to global norm <= 1 before Adam (here the norm is far above 1 with lam large)
    tr.l2 = 50.0
    tr.clip_gradients = True
    tr.loss_and_gradients(audio, lc, gc)
    g = tr.grads.cpu().numpy().astype(np.float64)
    nrm = np.sqrt((g ** 2).sum())
    assert nrm > 1.0
    p0 = tr.params.cpu().numpy().astype(np.float64)
    lr = tr.apply_gradients()
    gc_ = g / max(nrm, 1.0)
    p1, _, _, _ = R.adam_ema(p0, gc_, np.zeros_like(p0), np.zeros_like(p0), p0.copy(), 1, lr)
    np.testing.assert_allclose(tr.params.cpu().numpy(), p1, rtol=0, atol=2e-6)     # tolerance: one fp32 Adam update of size lr
    np.testing.assert_allclose(np.sqrt((tr.grads.cpu().numpy().astype(np.float64) ** 2).sum()), 1.0, rtol=1e-5)


def test_second_step_with_other_data_and_the_workspace_contract():
    """the fused layer kernels never write the activation rows in front of a layer's receptive offset again after the
    workspace's one-time clear and rely on them staying zero, so (1) nothing else may write into the carve: twv_wavenet_train_l2's
    scratch is a region of its own at the END of the workspace and clip_by_global_norm's is a separate buffer; (2) a second step with
    OTHER data on the same trainer gives bit for bit what a fresh trainer gives on that data (the step is run-to-run reproducible);
    (3) a caller that invalidated the workspace says so (reset_workspace) and gets a clean one."""
    dil = [1, 2, 4, 8, 1, 2]
    trA, tensors, cfg, audio, lc, gc = _case(dil=dil, B=3, Tm=4, seed=4)
    rng = np.random.RandomState(99)
    audio2 = ((rng.rand(*audio.shape) - 0.5) * 1.2).astype(np.float32)
    lc2 = (rng.randn(*lc.shape) * 0.7).astype(np.float32)
    gc2 = (1 - gc).astype(np.int32)
    trA.l2 = 0.01
    head0 = None
    trA.loss_and_gradients(audio, lc, gc)                       # first step: the workspace is cleared, L2 runs on it
    n = trA.n_params
    head = trA._ws[:n + 1024].clone()
    import ctypes as C
    from twvk_amd import _lib
    from twvk_amd.wavenet import _ptr, _stream
    with torch.cuda.device(trA.device):
        _lib.check(trA._L.twv_wavenet_train_l2(trA._h, _ptr(trA.params), 0.01, _ptr(trA._ws), _ptr(trA.loss), _ptr(trA.grads), _stream()))
    torch.cuda.synchronize()
    assert torch.equal(head, trA._ws[:n + 1024]), "twv_wavenet_train_l2 wrote into the start of the workspace (the carve of loss_grad)"
    trA.clip_gradients = True
    trA.apply_gradients()                                       # clipping uses its own scratch
    assert torch.equal(head, trA._ws[:n + 1024])
    # (2) second step, other data, same weights as a fresh trainer
    trB, _, _, _, _, _ = _case(dil=dil, B=3, Tm=4, seed=4)
    trA.load_weights(tensors); trA.l2 = 0.0
    lossA = float(trA.loss_and_gradients(audio2, lc2, gc2).item()); gA = trA.grads.clone()
    lossB = float(trB.loss_and_gradients(audio2, lc2, gc2).item()); gB = trB.grads.clone()
    assert lossA == lossB and torch.equal(gA, gB)
    l32, g32 = R.loss_and_grads(tensors, cfg, audio2, lc2, gc2)
    assert abs(lossA - l32) <= 1e-4 * abs(l32)
    # (3) a poisoned workspace after reset_workspace: cleared again, same bits
    trA._ws.fill_(float("nan"))
    trA.reset_workspace()
    lossC = float(trA.loss_and_gradients(audio2, lc2, gc2).item())
    assert lossC == lossB and torch.equal(trA.grads, gB)


def test_train_vocoder_cli_trains_checkpoints_and_resumes(tmp_path):
    """train_vocoder.py's loop on synthetic data: steps, a bundle every --checkpoint_every steps, at most hparams.max_checkpoints
    kept, and --logdir alone resumes from the last one (train_vocoder.py:133-152,175-176)"""
    import json
    import twvk_amd
    from twvk_amd import checkpoint as ckpt
    from twvk_amd.hparams import hparams
    from twvk_amd.train_vocoder import main as tv_main
    saved = {k: getattr(hparams, k) for k in ("dilations", "wavenet_batch_size", "sample_size", "skip_channels", "max_checkpoints")}
    try:
        hparams.dilations = [1, 2, 4, 8, 1, 2, 4, 8]; hparams.wavenet_batch_size = 2; hparams.sample_size = 1300
        hparams.skip_channels = 64; hparams.max_checkpoints = 2
        logdir = str(tmp_path / "run")
        lines = []
        r = tv_main(["--data_dir", "a,b", "--logdir", logdir, "--checkpoint_every", "2", "--num_steps", "6", "--synthetic"], log=lines.append)
        assert r["step"] == 6 and np.isfinite(r["loss"])
        assert sum(1 for l in lines if l.startswith("step ")) == 6
        kept = sorted(os.path.basename(p) for p in ckpt.all_checkpoint_paths(logdir))
        assert kept == ["model.ckpt-4", "model.ckpt-6"]                              # Saver(max_to_keep=2)
        assert not os.path.exists(os.path.join(logdir, "model.ckpt-2.index"))
        assert json.load(open(os.path.join(logdir, "params.json")))["wavenet_batch_size"] == 2
        lines = []
        r2 = tv_main(["--data_dir", "a,b", "--logdir", logdir, "--checkpoint_every", "100", "--num_steps", "8", "--synthetic"], log=lines.append)
        assert r2["step"] == 8 and any("Global step was: 6" in l for l in lines)    # resumed, two more steps
    finally:
        for k, v in saved.items():
            setattr(hparams, k, v)


def test_add_loss_and_add_optimizer_surface():
    """net.add_loss(...) / net.add_optimizer(hparams, global_step) (model.py:247,314) == WaveNetTrainer.step"""
    import twvk_amd
    tr, tensors, cfg, audio, lc, gc = _case(dil=[1, 2, 4, 1, 2], B=2, Tm=3)
    l_ref = float(tr.step(audio, lc, gc).item())
    p_ref = tr.params.cpu().numpy()
    net = make_model(2, [1, 2, 4, 1, 2], tensors, S=64)
    net._trainer_for(audio.shape[1]).load_weights(tensors)
    loss = net.add_loss(audio[:, :, None], lc, gc, l2_regularization_strength=0)
    lr = net.add_optimizer(twvk_amd.default_hparams(), 0)
    assert float(loss.item()) == l_ref and lr == pytest.approx(1e-3)
    assert np.array_equal(net._trainer.params.cpu().numpy(), p_ref)
