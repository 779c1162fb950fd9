"""The training step at residual_channels = dilation_channels = 64 and 128 on the MI355X (tr_layer_wide_fwd / bwd1 / bwd2_kernel and the
small kernels around them): every case of tests/train_wide_cases.py against the float64 torch restatement under the bars of the
width-32 step (RATIO 8, LOSS_FLOOR 2e-6, gradient floor FLOOR_G), the bit-level contracts of the step, the optimiser, and the loop
train -> save -> restore -> score -> generate at width 64.

A dead or swapped 32-channel block of a layer kernel shows as an error of order 1 of the tensor's maximum in that block's columns of
the layer's kernels, so the per-tensor comparison sees it (DESIGN 3c-w records the hand check)."""
import numpy as np
import pytest
import torch

import torch_train_ref as R
import train_wide_cases as TW
from train_cases import _assert_against_float64

pytestmark = pytest.mark.gpu


def _on_route(tr, W, want):
    route = tr.route()
    assert route["width"] == str(W) and {k: route[k] for k in want} == want, route


def _other_data(audio, lc, gc):
    rng = np.random.RandomState(99)
    return (((rng.rand(*audio.shape) - 0.5) * 1.2).astype(np.float32), (rng.randn(*lc.shape) * 0.7).astype(np.float32), (1 - gc).astype(np.int32))


# ---- (a) parity ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", TW.IDS)
def test_loss_and_gradients_against_float64(cid):
    _, W, kw, want = TW.BY_ID[cid]
    tensors, cfg, audio, lc, gc, q = TW.data(cid)
    tr = TW.trainer(cid)
    _on_route(tr, W, want)                                                # first: the case runs the kernels it is here for
    if q is not None:                                                     # the checker's class ids are the device quantizer's
        from twvk_amd.ops import mu_law_encode
        assert np.array_equal(mu_law_encode(torch.from_numpy(np.array(audio)).cuda(), kw["Q"]).cpu().numpy(), q)
    loss = float(tr.loss_and_gradients(audio, lc, gc).item())
    got = tr.gradients()
    l64, g64, l32, g32 = TW.reference(cid)
    _assert_against_float64(cid, loss, got, l64, g64, l32, g32, floor=TW.FLOOR_G)
    # the last layer's dense 1x1 has no path to the loss: exactly zero, not small
    last = "wavenet/dilated_stack/layer%d/dilation_layer/dense/" % (len(kw["dil"]) - 1)
    for k in [last + "kernel"] + ([last + "bias"] if kw.get("use_bias", True) else []):
        assert not g64[k].any(), k
        assert (got[k] == 0).all(), (cid, k, float(np.abs(got[k]).max()))
    if cid == "w64-g64-card5":
        emb64, emb = g64["wavenet/gc_embedding"], got["wavenet/gc_embedding"]
        used = sorted(set(kw["gc_ids"]))
        assert used == [0, 1, 3]
        for i in range(kw["gc_card"]):
            if i in used:
                assert np.abs(emb64[i]).max() > 0
            else:
                assert not emb64[i].any() and (emb[i] == 0).all(), i      # ids 2 and 4: no batch entry, exactly zero


# ---- (b) bits ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ["w64-small", "w64-staged", "w128-small", "w128-staged"])
def test_fresh_trainers_agree_and_a_second_step_equals_a_fresh_first(cid):
    _, _, audio, lc, gc, _ = TW.data(cid)
    audio2, lc2, gc2 = _other_data(audio, lc, gc)
    trA = TW.trainer(cid)
    lossA1 = float(trA.loss_and_gradients(audio, lc, gc).item()); gA1 = trA.grads.clone()
    trB = TW.trainer(cid)
    lossB1 = float(trB.loss_and_gradients(audio, lc, gc).item())
    assert lossA1 == lossB1 and torch.equal(gA1, trB.grads), "two fresh trainers, same data: different bits"
    lossA1b = float(trA.loss_and_gradients(audio, lc, gc).item())
    assert lossA1b == lossA1 and torch.equal(gA1, trA.grads), "the same step twice on one trainer: different bits"
    lossA2 = float(trA.loss_and_gradients(audio2, lc2, gc2).item()); gA2 = trA.grads.clone()       # other data on a used workspace
    trC = TW.trainer(cid)
    lossC = float(trC.loss_and_gradients(audio2, lc2, gc2).item())
    assert lossA2 == lossC and torch.equal(gA2, trC.grads), "a second step differs from a fresh trainer's first"
    assert lossA2 != lossA1 and np.isfinite(lossA2)


@pytest.mark.parametrize("cid", ["w64-small", "w128-hop32"])
def test_nan_filled_workspace_gives_the_bits_of_a_clean_one(cid):
    _, _, audio, lc, gc, _ = TW.data(cid)
    clean = TW.trainer(cid)
    loss0 = float(clean.loss_and_gradients(audio, lc, gc).item())
    tr = TW.trainer(cid)
    tr._ws.fill_(float("nan"))                                            # before the first step: the once-only clear takes it
    loss1 = float(tr.loss_and_gradients(audio, lc, gc).item())
    assert loss1 == loss0 and torch.equal(tr.grads, clean.grads)
    tr._ws.fill_(float("nan"))                                            # between steps: the caller says so
    tr.reset_workspace()
    loss2 = float(tr.loss_and_gradients(audio, lc, gc).item())
    assert loss2 == loss0 and torch.equal(tr.grads, clean.grads)


# ---- (c) optimiser -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ["w64-small", "w128-small"])
def test_twenty_steps_lower_the_loss(cid):
    _, _, audio, lc, gc, _ = TW.data(cid)
    tr = TW.trainer(cid)
    l0 = float(tr.step(audio, lc, gc).item())
    for _ in range(20):
        l1 = float(tr.step(audio, lc, gc).item())
    assert np.isfinite([l0, l1]).all() and l1 < l0, (l0, l1)
    assert tr.global_step == 21


@pytest.mark.parametrize("cid", ["w64-small", "w128-small"])
def test_l2_and_clipping_first_step_against_the_checker_then_steps(cid):
    """model.py:300-312 (L2 on the non-bias variables) and model.py:330-331 (clip_by_global_norm(gradients, 1.)) at the wide widths"""
    tensors, cfg, audio, lc, gc, _ = TW.data(cid)
    lam = 0.01
    tr = TW.trainer(cid, clip_gradients=True, l2_regularization_strength=lam)
    loss = float(tr.loss_and_gradients(audio, lc, gc).item())
    l64, g64, l32, g32 = TW.reference(cid)
    l2 = sum(0.5 * float((np.asarray(v, np.float64) ** 2).sum()) for k, v in tensors.items() if "bias" not in k)
    add = {k: (0.0 if "bias" in k else lam * np.asarray(tensors[k], np.float64)) for k in g64}
    _assert_against_float64(cid + " + L2", loss, tr.gradients(), l64 + lam * l2, {k: g64[k] + add[k] for k in g64}, l32 + lam * l2,
                            {k: g32[k] + add[k] for k in g64}, floor=TW.FLOOR_G)
    g = tr.grads.cpu().numpy().astype(np.float64)
    nrm = np.sqrt((g ** 2).sum())
    p0 = tr.params.cpu().numpy().astype(np.float64)
    lr = tr.apply_gradients()
    p1, _, _, _ = R.adam_ema(p0, g / max(nrm, 1.0), np.zeros_like(p0), np.zeros_like(p0), p0.copy(), 1, lr)
    np.testing.assert_allclose(tr.params.cpu().numpy(), p1, rtol=0, atol=2e-6)     # tolerance: one fp32 Adam update of size lr
    l0 = float(tr.step(audio, lc, gc).item())
    for _ in range(19):
        l1 = float(tr.step(audio, lc, gc).item())
    assert np.isfinite([l0, l1]).all() and l1 < l0, (l0, l1)


# ---- (d) the loop closed at width 64 -----------------------------------------------------------------------------------------------------
def test_train_save_restore_score_generate_at_64(tmp_path, oracle):
    from helpers import first_mismatch, mol_uniforms
    from twvk_amd.score import WaveNetScorer
    from twvk_amd.wavenet import WaveNetModel
    cid = "w64-small"
    _, W, kw, _ = TW.BY_ID[cid]
    tensors, cfg, audio, lc, gc, _ = TW.data(cid)
    tr = TW.trainer(cid)
    for _ in range(3):
        tr.step(audio, lc, gc)
    prefix = tr.save(str(tmp_path))
    # resume: a fresh trainer restored from the bundle takes the same next steps, bit for bit
    tr2 = TW.trainer(cid)
    assert tr2.restore(str(tmp_path)) == 3 and prefix.endswith("model.ckpt-3")
    assert torch.equal(tr2.params, tr.params) and torch.equal(tr2.m, tr.m) and torch.equal(tr2.v, tr.v) and torch.equal(tr2.ema, tr.ema)
    for _ in range(2):
        la, lb = float(tr.step(audio, lc, gc).item()), float(tr2.step(audio, lc, gc).item())
        assert la == lb
    assert torch.equal(tr2.params, tr.params) and torch.equal(tr2.ema, tr.ema) and tr2.global_step == 5
    # the trained weights in the scorer: held-out loss on the training batch against the float64 loss at those weights
    trained = tr.weights()
    hop, T = int(np.prod(kw.get("up", TW.UP))), audio.shape[1]
    sc = WaveNetScorer(TW.model(W, dict(kw, B=2), "cuda:0"), window=T, slots=2)
    sc.load_weights(trained)
    assert sc.route()["width"] == "64"
    mean, count = sc.held_out_loss([audio[i] for i in range(2)], [lc[i] for i in range(2)], [int(g) for g in gc])
    l64, _ = R.loss_and_grads(trained, cfg, audio, lc, gc, dtype=torch.float64)
    l32, _ = R.loss_and_grads(trained, cfg, audio, lc, gc, dtype=torch.float32)
    assert count == 2 * (T - R.receptive_field(cfg))
    assert abs(mean - l64) <= max(10 * abs(l32 - l64), TW.LOSS_FLOOR * abs(l64)), (mean, l32, l64)
    # and in the generation path: 300 steps at B = 1 on wn_wide_generate_kernel, bit for bit the CPU oracle
    O = oracle
    d = O.make_dims(kw["dil"], R=W, D=W, S=64, Q=256, out_channels=30, scalar_input=True, ifw=32, use_bias=True, G=32, gc_card=2, L=80, up=TW.UP)
    blob = O.blob_from_tensors(d, trained)
    m = WaveNetModel(1, kw["dil"], 2, W, W, 64, quantization_channels=256, out_channels=30, use_biases=True, scalar_input=True, initial_filter_width=32,
                     global_condition_channels=32, global_condition_cardinality=2, local_condition_channels=80, upsample_factor=list(TW.UP),
                     train_mode=False)
    m.load_weights(trained)
    assert m.kernel_name() == "wn_wide_generate_kernel"
    n = 300
    mel = np.array(lc[:1, :1])
    U_o = O.upsample(d, blob, mel)[:, :n].copy()
    U_g = m.create_upsample(mel)[:, :n].contiguous()
    g1, seed_in, u = np.array([int(gc[0])], np.int32), np.array([0.1], np.float32), mol_uniforms(1, n, 10)
    want = O.generate_mol(d, blob, O.State(d, 1), U_o, g1, seed_in, u)
    got = m.generate(U_g, g1, seed_in, u)
    assert np.abs(want).max() > 0 and first_mismatch(got.cpu().numpy(), want) is None


def test_train_vocoder_cli_at_width_64_writes_what_eval_vocoder_and_generate_read(tmp_path):
    """`python -m twvk_amd.train_vocoder` with residual_channels = dilation_channels = 64 in the hparams: steps, a bundle and a
    params.json with the widths; `eval_vocoder` scores files with it and `generate` vocodes a mel from it (both take the widths from
    params.json)"""
    import json
    from scipy.io import wavfile
    import twvk_amd
    from twvk_amd.eval_vocoder import main as eval_main
    from twvk_amd.generate import main as gen_main
    from twvk_amd.hparams import hparams
    from twvk_amd.train_vocoder import main as tv_main
    try:
        hparams.dilations = [1, 2, 4, 8, 1, 2, 4, 8]; hparams.wavenet_batch_size = 2; hparams.sample_size = 1300
        hparams.skip_channels = 64; hparams.residual_channels = hparams.dilation_channels = 64
        logdir = str(tmp_path / "run")
        lines = []
        r = tv_main(["--data_dir", "a,b", "--logdir", logdir, "--checkpoint_every", "2", "--num_steps", "4", "--synthetic"], log=lines.append)
        assert r["step"] == 4 and np.isfinite(r["loss"])
        saved = json.load(open(tmp_path / "run" / "params.json"))
        assert saved["residual_channels"] == 64 and saved["dilation_channels"] == 64
        rng = np.random.RandomState(3)
        dirs = [tmp_path / "spk0", tmp_path / "spk1"]
        for d, frames in zip(dirs, (2, 3)):
            d.mkdir()
            np.savez(str(d / "u0.npz"), audio=((rng.rand(frames * 300) - 0.5) * 1.6).astype(np.float32), mel=(rng.randn(frames, 80) * 0.5).astype(np.float32))
        got = eval_main(["--load_path", logdir, "--data_paths", ",".join(str(d) for d in dirs), "--window", "600", "--slots", "2"], log=lambda *_: None)
        assert got["count"] == 5 * 300 - 2 * 62 and np.isfinite(got["mean"])      # receptive field 32 + 30
        np.save(tmp_path / "mel.npy", rng.uniform(-4, 4, (1, 80)).astype(np.float32))
        paths = gen_main([logdir, "--mel", str(tmp_path / "mel.npy"), "--gc_cardinality", "2", "--gc_id", "1", "--batch_size", "1", "--seed", "3",
                          "--logdir", str(tmp_path / "log")])
        rate, wav = wavfile.read(paths[0])
        assert wav.shape == (300,) and np.abs(wav.astype(np.int64)).max() > 0
    finally:
        twvk_amd.hparams.__dict__.update(twvk_amd.default_hparams().__dict__)
