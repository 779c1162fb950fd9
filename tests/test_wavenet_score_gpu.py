"""WaveNet scoring on the GPU (score.py over twv_wavenet_score_windows / _reduce): every table case of tests/score_cases.py against the
float64 torch restatement of the reference's training graph on the WHOLE utterance, at every scored position; the mean against
float64 and against the training step; locality and repeatability bit for bit; independence of the window and slot count;
sensitivity to the head; stale memory; trained weights."""
import ctypes as C

import numpy as np
import pytest
import torch

import score_cases as SC
import train_cases as TC

pytestmark = pytest.mark.gpu


def _host(nll):
    return [v.cpu().numpy() for v in nll]


def _loss_bar(l, l64, l32):
    return abs(l - l64) <= max(10 * abs(l32 - l64), SC.LOSS_FLOOR * abs(l64))


# ---- per-sample parity: every case, every window, every utterance, every position ----------------------------------------------
@pytest.mark.parametrize("cid", SC.IDS)
def test_per_sample_nll_matches_float64_on_whole_utterances(cid):
    c = SC.case(cid)
    n64, n32 = SC.reference(cid)
    for wf in c.windows:
        sc = c.scorer(wf)
        assert {k: sc.route()[k] for k in c.route} == c.route, (cid, sc.route())           # the route first
        got = _host(sc.score(c.audios, c.mels, c.gcs))
        assert len(got) == len(c.audios)
        for i, g in enumerate(got):
            SC.assert_per_sample("%s window %d frames utterance %d" % (cid, wf, i), g, n64[i], n32[i])


@pytest.mark.parametrize("cid", SC.IDS)
def test_held_out_loss_matches_the_float64_mean(cid):
    c = SC.case(cid)
    l64, l32 = SC.means(cid)
    loss, count = c.scorer().held_out_loss(c.audios, c.mels, c.gcs)
    print("%s: held-out loss %.9f over %d samples (f64 %.9f, f32 %.9f)" % (cid, loss, count, l64, l32))
    assert count == sum(T - c.rf for T in c.lengths)
    assert _loss_bar(loss, l64, l32), (cid, loss, l64, l32)


def test_mean_of_a_uniform_batch_against_the_training_step():
    """B = 2, Tm = 3, one window each: the scored mean and twv_wavenet_train_loss_grad's loss on the same batch, both within the
    training step's loss bar of float64"""
    import torch_train_ref as R
    from twvk_amd.score import WaveNetScorer
    kw = dict(TC.DEFAULT_CASES)["small"]
    tr, tensors, cfg, audio, lc, gc = TC._case(**kw)
    l64, _ = R.loss_and_grads(tensors, cfg, audio, lc, gc, dtype=torch.float64)
    l32, _ = R.loss_and_grads(tensors, cfg, audio, lc, gc, dtype=torch.float32)
    l_train = float(tr.loss_and_gradients(audio, lc, gc).item())
    sc = WaveNetScorer(tr.net, window=audio.shape[1], slots=2)
    sc.load_weights(tr.params)                                    # the trainer's flat blob as it is
    l_score, count = sc.held_out_loss(list(audio), list(lc), gc)
    print("uniform batch: scored %.9f, training step %.9f, f64 %.9f, f32 %.9f" % (l_score, l_train, l64, l32))
    assert count == 2 * tr.output_width
    assert _loss_bar(l_train, l64, l32) and _loss_bar(l_score, l64, l32), (l_score, l_train, l64, l32)


# ---- locality and repeatability, bit for bit -------------------------------------------------------------------------------------
def test_locality_bit_for_bit():
    """scoring twice gives equal bits; changing audio[j] of one utterance leaves every nll[t] with t < j or t > j + rf equal bit for bit
    in every utterance and changes nll[j].  j in the interior of the second window (start 600, kept 1800 .. 2399) of the 9-frame
    utterance of `one-cycle`, and j = rf: a wrong halo, a wrong kept range or slot cross-talk shows here."""
    c = SC.case("one-cycle")
    sc = c.scorer()
    base = _host(sc.score(c.audios, c.mels, c.gcs))
    again = _host(sc.score(c.audios, c.mels, c.gcs))
    for a, b in zip(base, again):
        assert a.tobytes() == b.tobytes()
    rf = c.rf
    for j in (2000, rf):
        audios = [a.copy() for a in c.audios]
        audios[1][j] = -audios[1][j] if abs(audios[1][j]) > 0.05 else 0.4
        got = _host(sc.score(audios, c.mels, c.gcs))
        assert got[0].tobytes() == base[0].tobytes(), j
        t = np.arange(rf, c.lengths[1])
        outside = (t < j) | (t > j + rf)
        assert outside.sum() > 0 and (~outside).sum() == min(rf + 1, c.lengths[1] - j)
        assert got[1][outside].tobytes() == base[1][outside].tobytes(), j
        assert got[1][j - rf] != base[1][j - rf], j
        assert (got[1][~outside] != base[1][~outside]).sum() > 16, j                      # ... and so do the positions whose first convolution sees it


# ---- window independence ------------------------------------------------------------------------------------------------------------
def test_window_and_slot_count_do_not_matter():
    c = SC.case("hop64")
    n64, n32 = SC.reference("hop64")
    runs = {}
    for wf in c.windows:
        for slots in (1, 3, 8):
            got = _host(c.scorer(wf, slots=slots).score(c.audios, c.mels, c.gcs))
            for i, g in enumerate(got):
                SC.assert_per_sample("hop64 window %d slots %d utterance %d" % (wf, slots, i), g, n64[i], n32[i])
            runs[(wf, slots)] = got
    first = runs[(c.windows[0], 1)]
    for key, got in sorted(runs.items()):
        same = all(a.tobytes() == b.tobytes() for a, b in zip(first, got))
        worst = max(float(np.abs(a.astype(np.float64) - b).max()) for a, b in zip(first, got))
        print("window %d frames, %d slots against window %d, 1 slot: bits %s (max difference %.3g)" % (key + (c.windows[0], "agree" if same else "differ", worst)))


# ---- sensitivity: the output comes from the head -------------------------------------------------------------------------------------
def _mol_nll64(y, tgt):
    """mixture.py:27-81 for ONE parameter row y (3 nr) against targets tgt (n), float64 numpy -> (n,)"""
    nr = len(y) // 3
    logit, mu, ls = y[:nr], y[nr:2 * nr], np.maximum(y[2 * nr:], np.log(1e-14))
    sp = lambda x: np.logaddexp(0.0, x)
    sig = lambda x: 1.0 / (1.0 + np.exp(-x))
    cen = tgt[:, None] - mu[None]
    inv = np.exp(-ls)[None]
    plus, mn, mid = inv * (cen + 1.0 / 65535), inv * (cen - 1.0 / 65535), inv * cen
    delta = sig(plus) - sig(mn)
    t = tgt[:, None]
    lp = np.where(t < -0.999, plus - sp(plus), np.where(t > 0.999, -sp(mn), np.where(delta > 1e-5, np.log(np.maximum(delta, 1e-12)),
                                                                                   mid - ls[None] - 2.0 * sp(mid) - np.log(65535 / 2.0))))
    lp = lp + (logit - np.logaddexp.reduce(logit))[None]
    return -np.logaddexp.reduce(lp, axis=1)


def test_zeroed_output_kernel_gives_the_bias_only_mixture():
    c = SC.case("small")
    tensors = dict(c.tensors)
    tensors["wavenet/conv1d_2/kernel"] = np.zeros_like(tensors["wavenet/conv1d_2/kernel"])
    got = _host(c.scorer(tensors=tensors).score(c.audios, c.mels, c.gcs))
    bias = np.asarray(tensors["wavenet/conv1d_2/bias"], np.float64)
    plain = _host(c.scorer().score(c.audios, c.mels, c.gcs))
    for i, g in enumerate(got):
        want = _mol_nll64(bias, c.audios[i][c.rf:].astype(np.float64))
        assert np.abs(g - want).max() <= 1e-5, (i, np.abs(g - want).max())
        assert np.abs(plain[i] - want).max() > 1e-3                  # with its kernel the head says something else


# ---- stale memory ----------------------------------------------------------------------------------------------------------------------
def test_nan_filled_workspace_and_output_change_nothing():
    """`small-shifted`: a short slot next to a full one, and an idle slot in the last batch.  Every batch is run on a zeroed and on a
    NaN-filled workspace and nll buffer: the positions a slot has are finite and equal bit for bit, the others are written as 0."""
    from twvk_amd import score as S
    c = SC.case("small-shifted")
    sc = c.scorer()
    table = S.plan(c.lengths, sc.window, c.rf, c.hop, sc.slots).table
    assert (table[-1, :, S.UTT] < 0).any() and len({int(n) for n in table[:, :, S.LENGTH].ravel() if n > 0}) > 1
    for rows in table:
        staged = sc.stage(rows, c.audios, c.mels, c.gcs)
        sc.run(*staged)                                               # allocates the workspace
        sc._ws.zero_()
        clean = sc.run(*staged, nll=torch.zeros((sc.slots, sc.width), device=sc.device)).cpu().numpy()
        sc._ws.fill_(float("nan"))
        dirty = sc.run(*staged, nll=torch.full((sc.slots, sc.width), float("nan"), device=sc.device)).cpu().numpy()
        assert np.isfinite(dirty).all()
        assert dirty.tobytes() == clean.tobytes()
        for s, (u, _, n, _, _) in enumerate(rows):
            have = max(int(n) - c.rf, 0) if u >= 0 else 0
            assert (dirty[s, :have] > 0).all() and not dirty[s, have:].any(), (s, have)


# ---- trained weights -------------------------------------------------------------------------------------------------------------------
def test_held_out_loss_falls_with_training():
    """30 steps of the small training case; the scorer on tr.params and on tr.ema, on the training batch: both below the value at
    initialisation, and the raw weights (30 Adam steps) below the EMA shadows (decay 0.9999: they have barely moved)"""
    from twvk_amd.score import WaveNetScorer
    kw = dict(TC.DEFAULT_CASES)["small"]
    tr, tensors, cfg, audio, lc, gc = TC._case(**kw)
    sc = WaveNetScorer(tr.net, window=audio.shape[1], slots=2)
    sc.load_weights(tensors)
    before, _ = sc.held_out_loss(list(audio), list(lc), gc)
    for _ in range(30):
        tr.step(audio, lc, gc)
    sc.load_weights(tr.params)
    raw, _ = sc.held_out_loss(list(audio), list(lc), gc)
    sc.load_weights(tr.ema)
    ema, _ = sc.held_out_loss(list(audio), list(lc), gc)
    print("held-out loss on the training batch: at initialisation %.6f, after 30 steps %.6f (raw), %.6f (EMA)" % (before, raw, ema))
    assert raw < ema < before, (before, raw, ema)


# ---- the eval_vocoder tool -------------------------------------------------------------------------------------------------------------
def test_eval_vocoder_restores_raw_variables_or_ema_shadows(tmp_path):
    """`python -m twvk_amd.eval_vocoder`: a bundle with raw variables and different EMA shadows, two speaker directories; the printed
    means are those of WaveNetScorer on the files' utterances (audio cut to frames * hop) with the raw weights, and with --ema the shadows"""
    import json
    import twvk_amd
    from twvk_amd import checkpoint as ck, weights as W
    from twvk_amd.eval_vocoder import main
    from twvk_amd.score import WaveNetScorer
    dil = [1, 2, 4, 8]
    logdir = tmp_path / "ckpt"; logdir.mkdir()
    json.dump({"dilations": dil, "skip_channels": 64}, open(logdir / "params.json", "w"))
    specs = W.tensor_specs(len(dil), S=64)
    raw, ema = W.random_tensors(specs, seed=21), W.random_tensors(specs, seed=22)
    var = dict(raw)
    var.update({k + ck.EMA_SUFFIX: v for k, v in ema.items()})
    var["global_step"] = np.asarray(5, np.int32)
    ck.write_bundle(str(logdir / "model.ckpt-5"), var)
    ck.write_checkpoint_state(str(logdir), str(logdir / "model.ckpt-5"))
    rng = np.random.RandomState(3)
    dirs, utts = [tmp_path / "spk0", tmp_path / "spk1"], []
    for spk, (d, frames) in enumerate(zip(dirs, ([2, 5], [4]))):
        d.mkdir()
        for k, f in enumerate(frames):
            audio, mel = ((rng.rand(f * 300 + 17 * k) - 0.5) * 1.6).astype(np.float32), (rng.randn(f, 80) * 0.5).astype(np.float32)
            np.savez(str(d / ("u%d.npz" % k)), audio=audio, mel=mel)
            utts.append((spk, audio[:f * 300], mel))
    try:
        args = ["--load_path", str(logdir), "--data_paths", ",".join(str(d) for d in dirs), "--window", "900", "--slots", "2"]
        out_file = tmp_path / "per.txt"
        got_raw = main(args + ["--per_utterance_out", str(out_file)], log=lambda *_: None)
        got_ema = main(args + ["--ema"], log=lambda *_: None)
    finally:
        twvk_amd.hparams.__dict__.update(twvk_amd.default_hparams().__dict__)
    net = TC._model(B=2, dil=dil, S=64, use_bias=True, up=TC.UP, out_channels=30, ifw=32, G=32, gc_card=2, scalar_input=True, Q=256, device="cuda:0")
    sc = WaveNetScorer(net, window=900, slots=2)
    for tensors, got in ((raw, got_raw), (ema, got_ema)):
        sc.load_weights(tensors)
        want = _host(sc.score([u[1] for u in utts], [u[2] for u in utts], [u[0] for u in utts]))
        n = sum(w.size for w in want)
        assert got["count"] == n == sum(len(u[1]) - net.receptive_field for u in utts)
        assert abs(got["mean"] - float(np.concatenate(want).astype(np.float64).mean())) <= 1e-9 * got["mean"]
        assert [r[2] for r in got["rows"]] == [w.size for w in want] and sorted(got["per_dir"]) == [0, 1]
    assert abs(got_raw["mean"] - got_ema["mean"]) > 1e-4
    lines = open(out_file).read().splitlines()
    assert len(lines) == 3 and lines[0].split("\t")[:3] == ["0", str(dirs[0] / "u0.npz"), str(2 * 300 - net.receptive_field)]
