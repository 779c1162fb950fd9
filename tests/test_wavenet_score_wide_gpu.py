"""WaveNet scoring at residual_channels = dilation_channels = 64 and 128 on the GPU (sc_layer_wide_fwd_kernel under score.py): every
table case of tests/score_wide_cases.py against the float64 checker on the WHOLE utterance at every scored position, the held-out
mean, and -- because the NLL cannot see a wrong channel -- every layer's z rows and the raw output through twv_wavenet_score_view
against the checker on the same crop; slot independence, repeatability and stale memory bit for bit; window and slot count;
eval_vocoder on a width-64 logdir."""
import json

import numpy as np
import pytest
import torch

import score_cases as SC
import score_wide_cases as WC

pytestmark = pytest.mark.gpu


def _host(nll):
    return [v.cpu().numpy() for v in nll]


# ---- per-sample parity and the views ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", WC.IDS)
def test_per_sample_nll_matches_float64_on_whole_utterances(cid):
    c = WC.case(cid)
    n64, n32 = WC.reference(cid)
    for wf in c.windows:
        sc = c.scorer(wf)
        assert {k: sc.route()[k] for k in c.route} == c.route, (cid, sc.route())           # the route first
        got = _host(sc.score(c.audios, c.mels, c.gcs))
        assert len(got) == len(c.audios)
        for i, g in enumerate(got):
            SC.assert_per_sample("%s window %d frames utterance %d" % (cid, wf, i), g, n64[i], n32[i])


@pytest.mark.parametrize("cid", WC.IDS)
def test_held_out_loss_matches_the_float64_mean(cid):
    c = WC.case(cid)
    l64, l32 = WC.means(cid)
    loss, count = c.scorer().held_out_loss(c.audios, c.mels, c.gcs)
    print("%s: held-out loss %.9f over %d samples (f64 %.9f, f32 %.9f)" % (cid, loss, count, l64, l32))
    assert count == sum(T - c.rf for T in c.lengths)
    assert abs(loss - l64) <= max(10 * abs(l32 - l64), SC.LOSS_FLOOR * abs(l64)), (cid, loss, l64, l32)


@pytest.mark.parametrize("cid", WC.IDS)
def test_every_layer_s_z_and_the_output_match_float64(cid):
    """after the first window batch: ZC[:, l W : (l + 1) W] of every layer and Y, rows p < len_b - rf of every live slot, against the
    checker on the slot's crop: e = max|. - .64| / max|.64| per layer (per slot for y), e <= max(8 e_t32, FLOOR_Z).  A dead or
    swapped channel is about 1e5 bars away (every channel has max|z| >= 0.38 of its layer's maximum)."""
    c = WC.case(cid)
    sc = c.scorer()
    rows = WC.first_batch(c)
    assert (rows[:, 0] >= 0).any()
    sc.run(*sc.stage(rows, c.audios, c.mels, c.gcs))
    ez, ey = WC.view_errors(c, sc, rows)
    assert len(ez) == c.n_layers and len(ey) == int((rows[:, 0] >= 0).sum())
    WC.assert_views(cid, ez, ey)


# ---- bit for bit -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ["w64-small", "w128-one-cycle"])
def test_a_slot_does_not_depend_on_the_other_slots_and_runs_repeat(cid):
    """two runs give equal bits; with every OTHER utterance replaced (its audio negated, its mel reversed, the other speaker) an
    utterance's values and its slot's z rows keep their bits: no slot reaches its neighbour's rows"""
    c = WC.case(cid)
    sc = c.scorer()
    base = _host(sc.score(c.audios, c.mels, c.gcs))
    again = _host(sc.score(c.audios, c.mels, c.gcs))
    for a, b in zip(base, again):
        assert a.tobytes() == b.tobytes()
    audios = [a if i == 0 else -a for i, a in enumerate(c.audios)]
    mels = [m if i == 0 else m[::-1].copy() for i, m in enumerate(c.mels)]
    gcs = [g if i == 0 else 1 - g for i, g in enumerate(c.gcs)]
    got = _host(sc.score(audios, mels, gcs))
    assert got[0].tobytes() == base[0].tobytes()
    assert all(g.tobytes() != b.tobytes() for g, b in zip(got[1:], base[1:]))
    # the same through the view: slot 0 of the first batch holds utterance 0
    rows = WC.first_batch(c)
    assert rows[0, 0] == 0 and rows[1, 0] > 0
    have = (int(rows[0, 2]) - c.rf)
    sc.run(*sc.stage(rows, c.audios, c.mels, c.gcs))
    z0, y0 = sc.view("zc")[:have].cpu().numpy(), sc.view("y")[:have].cpu().numpy()
    sc.run(*sc.stage(rows, audios, mels, gcs))
    assert sc.view("zc")[:have].cpu().numpy().tobytes() == z0.tobytes() and sc.view("y")[:have].cpu().numpy().tobytes() == y0.tobytes()
    assert np.abs(z0).max(axis=0).min() > 0.0


@pytest.mark.parametrize("cid", ["w64-hop32", "w128-hop32"])
def test_window_and_slot_count_do_not_matter(cid):
    """as test_wavenet_score_gpu.py holds it at 32: every (window, slots) pair holds the per-sample bar, and so do the z rows of the
    first window through the view; whether the bits agree is printed (the front's and the head's library GEMMs may pick another kernel
    at another row count)"""
    c = WC.case(cid)
    n64, n32 = WC.reference(cid)
    runs = {}
    for wf in c.windows:
        for slots in (1, 3):
            sc = c.scorer(wf, slots=slots)
            got = _host(sc.score(c.audios, c.mels, c.gcs))
            for i, g in enumerate(got):
                SC.assert_per_sample("%s window %d slots %d utterance %d" % (cid, wf, slots, i), g, n64[i], n32[i])
            runs[(wf, slots)] = got
            rows = WC.first_batch(c, wf, slots)
            sc.run(*sc.stage(rows, c.audios, c.mels, c.gcs))
            WC.assert_views("%s window %d slots %d" % (cid, wf, slots), *WC.view_errors(c, sc, rows))
    first = runs[(c.windows[0], 1)]
    for key, got in sorted(runs.items()):
        same = all(a.tobytes() == b.tobytes() for a, b in zip(first, got))
        print("%s window %d frames, %d slots against window %d, 1 slot: nll bits %s" % ((cid,) + key + (c.windows[0], "agree" if same else "differ")))


@pytest.mark.parametrize("cid", ["w64-small", "w128-small", "w128-staged"])
def test_nan_filled_workspace_and_output_change_nothing(cid):
    """`small`: a short slot next to a full one and an idle slot in the last batch; `staged`: the other lc route.  Every batch on a zeroed and on a NaN-filled
    workspace and nll buffer: the positions a slot has are finite and equal bit for bit, as are its z rows; the others are written as 0."""
    from twvk_amd import score as S
    c = WC.case(cid)
    sc = c.scorer()
    table = S.plan(c.lengths, sc.window, c.rf, c.hop, sc.slots).table
    if "small" in cid:
        assert (table[-1, :, S.UTT] < 0).any() and len({int(n) for n in table[:, :, S.LENGTH].ravel() if n > 0}) > 1
    for rows in table:
        staged = sc.stage(rows, c.audios, c.mels, c.gcs)
        sc.run(*staged)                                               # allocates the workspace
        sc._ws.zero_()
        clean = sc.run(*staged, nll=torch.zeros((sc.slots, sc.width), device=sc.device)).cpu().numpy()
        zclean = sc.view("zc").cpu().numpy()
        sc._ws.fill_(float("nan"))
        dirty = sc.run(*staged, nll=torch.full((sc.slots, sc.width), float("nan"), device=sc.device)).cpu().numpy()
        zdirty = sc.view("zc").cpu().numpy()
        assert np.isfinite(dirty).all()
        assert dirty.tobytes() == clean.tobytes()
        for s, (u, _, n, _, _) in enumerate(rows):
            have = max(int(n) - c.rf, 0) if u >= 0 else 0
            assert (dirty[s, :have] > 0).all() and not dirty[s, have:].any(), (s, have)
            lo = s * sc.width
            assert zdirty[lo:lo + have].tobytes() == zclean[lo:lo + have].tobytes()
            assert np.isnan(zdirty[lo + have:lo + sc.width]).all()    # rows the slot does not have are not written


# ---- the eval_vocoder tool at width 64 ---------------------------------------------------------------------------------------------
def test_eval_vocoder_scores_a_width_64_logdir(tmp_path):
    """params.json says residual_channels = dilation_channels = 64: the tool's per-utterance and overall means are WaveNetScorer's on
    the same files, bit for bit"""
    import twvk_amd
    from twvk_amd import checkpoint as ck, weights as W
    from twvk_amd.eval_vocoder import main
    from twvk_amd.score import WaveNetScorer
    dil = [1, 2, 4, 8]
    logdir = tmp_path / "ckpt"; logdir.mkdir()
    json.dump({"dilations": dil, "skip_channels": 64, "residual_channels": 64, "dilation_channels": 64}, open(logdir / "params.json", "w"))
    specs = W.tensor_specs(len(dil), 64, 64, S=64)
    raw = W.random_tensors(specs, seed=31)
    var = dict(raw)
    var["global_step"] = np.asarray(7, np.int32)
    ck.write_bundle(str(logdir / "model.ckpt-7"), var)
    ck.write_checkpoint_state(str(logdir), str(logdir / "model.ckpt-7"))
    rng = np.random.RandomState(5)
    dirs, utts = [tmp_path / "spk0", tmp_path / "spk1"], []
    for spk, (d, frames) in enumerate(zip(dirs, ([2, 5], [4]))):
        d.mkdir()
        for k, f in enumerate(frames):
            audio, mel = ((rng.rand(f * 300 + 11 * k) - 0.5) * 1.6).astype(np.float32), (rng.randn(f, 80) * 0.5).astype(np.float32)
            np.savez(str(d / ("u%d.npz" % k)), audio=audio, mel=mel)
            utts.append((spk, audio[:f * 300], mel))
    try:
        got = main(["--load_path", str(logdir), "--data_paths", ",".join(str(d) for d in dirs), "--window", "900", "--slots", "2"], log=lambda *_: None)
    finally:
        twvk_amd.hparams.__dict__.update(twvk_amd.default_hparams().__dict__)
    net = WC.wide_model(64, B=2, dil=dil, S=64, use_bias=True, up=WC.UP, out_channels=30, ifw=32, G=32, gc_card=2, scalar_input=True, Q=256, device="cuda:0")
    sc = WaveNetScorer(net, window=900, slots=2)
    assert sc.route()["width"] == "64"
    sc.load_weights(raw)
    want = sc.score([u[1] for u in utts], [u[2] for u in utts], [u[0] for u in utts])
    assert [r[2] for r in got["rows"]] == [int(w.numel()) for w in want]
    assert [r[3] for r in got["rows"]] == [float(w.double().mean().item()) for w in want]          # bit for bit
    n = sum(int(w.numel()) for w in want)
    assert got["count"] == n and got["mean"] == sum(int(w.numel()) * float(w.double().mean().item()) for w in want) / n
    assert 5.0 < got["mean"] < 20.0
