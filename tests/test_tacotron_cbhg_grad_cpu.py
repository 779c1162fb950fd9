"""-m "not gpu": the host side of the Tacotron encoder / post-net gradients -- the checker itself (tests/torch_tacotron_cbhg_grad_ref.py:
the forward restatement bit for bit, autograd anchored by central differences, the tie rule of the max pool, the float32 yardstick), the
margin condition of every case of the GPU table, the linear-loss cotangent, the exported symbols, every refusal of the new entries (all
before a device is looked at), the unchanged size of the inference workspace and the two new views."""
import ctypes as C

import numpy as np
import pytest

from tacotron_cbhg_grad_cases import CASES, CHAIN_CASES, CHAIN_E_T32, MARGIN, SMALL, hparams, host_case

MAX_ITERS = 8
WS_CASES = ((1, 1), (8, 45), (32, 101), (32, 512), (64, 1024))          # tests/test_tacotron_grad_cpu.py: the parent's sizes
WS_PARENT = (29493568, 231162176, 925958464, 952893760, 2014576960)


def _model(num_speakers=2, **kw):
    from twvk_amd.tacotron import Tacotron
    return Tacotron(hparams(max_iters=MAX_ITERS, **dict(SMALL, **kw)), num_speakers=num_speakers)


@pytest.fixture(scope="module")
def model():
    return _model()


def test_restated_forward_is_the_restatement_bit_for_bit():
    import torch
    import torch_tacotron_cbhg_grad_ref as CG
    import torch_tacotron_grad_ref as G
    import torch_tacotron_ref as R
    import torch_tacotron_targets_ref as TR
    for name in ("A-masked-tails", "E-single-speaker", "F-speaker-tables"):
        h = host_case(name)
        memory = CG.encoder_vjp(h.w, h.enc_names, h.dims, h.tok, h.ln, *CG.speaker_side(h.w, h.dims, h.spk)[:2])[0]
        if "speaker_embedding" in h.w or h.speakers == 1:
            assert np.array_equal(memory, G.encoder_side(h.w, h.dims, h.tok, h.ln, h.spk)[0]), name
        mel64, lin_ref, _ = TR.forward_targets(h.w, h.dims, h.tok, h.ln, h.spk, h.at, h.tgt, h.TO, True)
        linear = CG.postnet_vjp(h.w, h.post_names, h.dims, mel64)[0]
        assert linear.dtype == np.float64 and np.array_equal(linear, lin_ref), name
        with torch.no_grad():       # and the CBHG alone against torch_tacotron_ref._cbhg
            w64 = {k: R._t(v) for k, v in h.w.items()}
            x = torch.as_tensor(mel64)
            a = R._cbhg(x, None, w64, "post_cbhg", h.dims.post_bank, 2, h.dims.post_hw_depth)
            b = CG._cbhg(x, None, w64, "post_cbhg", h.dims.post_bank, 2, h.dims.post_hw_depth)
            assert torch.equal(a, b), name


def test_checker_gradients_agree_with_central_differences():
    """float64, eps = 1e-6, three random directions over all leaves at once: (f(x + eps d) - f(x - eps d)) / (2 eps) against g . d, relative
    1e-6 as tests/test_tacotron_grad_cpu.py holds the decoder's (f = <output, cotangent>)"""
    import torch_tacotron_cbhg_grad_ref as CG
    h = host_case("A-masked-tails")
    eps, rng = 1e-6, np.random.RandomState(5)
    d_mem, d_lin = h.d_memory.astype(np.float64) * 1e3, h.d_linear.astype(np.float64) * 1e3
    _, ge, _ = CG.encoder_vjp(h.w, h.enc_names, h.dims, h.tok, h.ln, h.bh, h.init, d_mem)
    _, gp, _ = CG.postnet_vjp(h.w, h.post_names, h.dims, h.mel, d_lin)

    def full(name, g):           # a batch norm's (d_gamma, d_beta) against directions in (gamma, beta) only
        return np.concatenate([g, np.zeros_like(g)]) if name.endswith("batch_normalization") else g
    for _ in range(3):
        base = {k: np.asarray(h.w[k], np.float64) for k in h.enc_names + h.post_names}
        dirs = {k: rng.randn(*base[k].shape) * (np.arange(base[k].shape[0])[:, None] < 2 if k.endswith("batch_normalization") else 1.0) for k in base}
        dirs["embedding"][0] = 0.0
        db, di, dm = rng.randn(*h.bh.shape), rng.randn(*h.init.shape), rng.randn(*h.mel.shape)

        def fe(s):
            w = {k: base[k] + s * eps * dirs[k] for k in h.enc_names}
            return float((CG.encoder_vjp(w, h.enc_names, h.dims, h.tok, h.ln, h.bh + s * eps * db, h.init + s * eps * di)[0] * d_mem).sum())

        def fp(s):
            w = {k: base[k] + s * eps * dirs[k] for k in h.post_names}
            return float((CG.postnet_vjp(w, h.post_names, h.dims, h.mel + s * eps * dm)[0] * d_lin).sum())
        for label, f, gd in (("encoder", fe, sum(float((full(k, ge[k]) * dirs[k]).sum()) for k in h.enc_names)
                              + float((ge["d_before_highway"] * db).sum()) + float((ge["d_rnn_init"] * di).sum())),
                             ("post net", fp, sum(float((full(k, gp[k]) * dirs[k]).sum()) for k in h.post_names) + float((gp["d_mel"] * dm).sum()))):
            fd = (f(+1) - f(-1)) / (2 * eps)
            print("%s: central difference %.12e, g . d %.12e, relative %.2e" % (label, fd, gd, abs(fd - gd) / abs(gd)))
            assert abs(fd - gd) <= 1e-6 * abs(gd), (label, fd, gd)


def test_a_tie_at_the_max_pool_goes_to_the_earlier_position():
    import torch
    import torch_tacotron_cbhg_grad_ref as CG
    x = torch.tensor([[[1.0], [1.0], [3.0], [2.0], [2.0], [2.0], [0.5]]], dtype=torch.float64, requires_grad=True)
    rec = CG.new_record()
    y = CG._max_pool2(x, rec)
    assert y[0, :, 0].tolist() == [1.0, 3.0, 3.0, 2.0, 2.0, 2.0, 0.5]
    y.backward(torch.tensor([[[1.0], [10.0], [100.0], [1e3], [1e4], [1e5], [1e6]]], dtype=torch.float64))
    # windows {0,1} tie -> 0; {1,2} -> 2; {2,3} -> 2; {3,4} tie -> 3; {4,5} tie -> 4; {5,6} -> 5; {6} -> 6
    assert x.grad[0, :, 0].tolist() == [1.0, 0.0, 110.0, 1e3, 1e4, 1e5, 1e6]
    assert rec["pool_gap"] == 1.0
    # torch.maximum would have split the ties
    x2 = x.detach().clone().requires_grad_(True)
    torch.maximum(x2[:, :-1], x2[:, 1:]).sum().backward()
    assert x2.grad[0, 0, 0].item() == 0.5


def test_float32_yardstick_is_close_to_float64():
    h = host_case("A-masked-tails")
    for run in (h.encoder_checker, h.postnet_checker):
        o64, g64, _ = run("float64")
        o32, g32, _ = run("float32")
        assert o32.dtype == np.float32 and all(v.dtype == np.float32 for v in g32.values())
        worst = max(float(np.abs(g32[k] - g64[k]).max()) / float(np.abs(g64[k]).max()) for k in g64)
        assert 0.0 < worst < 1e-4, worst
        assert not g64.get("embedding", np.zeros((1, 1)))[0].any()


@pytest.mark.parametrize("name", sorted(CASES))
def test_margin_condition_of_the_gpu_table(name):
    """the float64 and the float32 checker run of a case take the same branch at every relu and make the same choice at every pool window
    between live values, and stay MARGIN clear of every edge: a comparison across a flipped branch would mean nothing"""
    same, relu_margin, pool_gap = host_case(name).margins()
    print("%s: relu margin %.3e, pool gap %.3e" % (name, relu_margin, pool_gap))
    assert same and relu_margin > MARGIN and pool_gap > MARGIN, (name, same, relu_margin, pool_gap)


@pytest.mark.parametrize("name", CHAIN_CASES)
def test_margin_condition_of_the_chain_cases(name):
    """the same for the whole-model runs the chain test compares against, with the sign of every output - target difference beyond the
    reach of float32 rounding, the attention clamps clear of their edges and every tensor's float32 yardstick a measure, not noise"""
    import torch_tacotron_cbhg_grad_ref as CG
    h = host_case(name)
    _, _, _, g64, rec = h.chain_checker("float64")
    _, _, _, g32, rec32 = h.chain_checker("float32")
    assert CG.same_branches(rec, rec32) and rec["relu_margin"] > MARGIN and rec["pool_gap"] > MARGIN, (rec["relu_margin"], rec["pool_gap"])
    assert rec["loss_margin"] > 1e-5 and rec["cumprod_margin"] > 1e-3 and rec["min_one_minus_p"] >= np.finfo(np.float32).tiny, rec["loss_margin"]
    worst = max((float(np.abs(g32[k] - g64[k]).max()) / max(float(np.abs(g64[k]).max()), 1e-30), k) for k in g64)
    print("%s: worst e_t32 %.3e (%s)" % ((name,) + worst))
    assert worst[0] < CHAIN_E_T32, worst
    assert set(g64) == set(CG.model_names(h.specs)) | {"d_init"} | ({"d_before_highway", "d_encoder_rnn_init"} if h.speakers > 1 else set())


@pytest.mark.parametrize("prioritize", [False, True])
def test_linear_loss_cotangent_is_the_derivative_of_add_loss(prioritize):
    """autograd of the restated loss lines against the closed form of the header, and against torch_tacotron_targets_ref.add_loss by
    central differences (the loss is piecewise linear: exact up to rounding away from a kink)"""
    import torch_tacotron_cbhg_grad_ref as CG
    import torch_tacotron_targets_ref as TR
    h = host_case("A-masked-tails")
    rng = np.random.RandomState(9)
    N, TO, F, sr = h.N, 6, h.hp.num_freq, float(h.hp.sample_rate)
    lin, tgt = rng.uniform(-4, 4, (N, TO, F)).astype(np.float32), rng.uniform(-4, 4, (N, TO, F)).astype(np.float32)
    lin, tgt = np.round(lin * 1024) / 1024, np.round(tgt * 1024) / 1024      # (on a 2^-10 grid, so that the stepped values below are float32 too)
    tgt[0, 0, :5] = lin[0, 0, :5]
    mel = np.zeros((N, TO, 1), np.float32)
    got = CG.linear_loss_cotangent(lin, tgt, h.coeff, prioritize, sr, F)
    lo, hi = int(165 / (sr * 0.5) * F), int(5000 / (sr * 0.5) * F)
    s = np.sign(lin.astype(np.float64) - tgt) * h.coeff.astype(np.float64)[:, None, None]
    band = ((np.arange(F) >= lo) & (np.arange(F) < hi)).astype(np.float64)
    want = s * (0.5 / (N * TO * F) + band * 0.5 / (N * TO * (hi - lo))) if prioritize else s / (N * TO * F)
    assert 0 < lo < hi < F and np.allclose(got, want, rtol=1e-12, atol=0) and not got[0, 0, :5].any()
    d = np.clip(rng.randn(N, TO, F), -4, 4) * (np.abs(lin - tgt) > 0.05)        # (steps of at most 2^-8 stay on their side of every kink)
    f = lambda e: TR.add_loss(mel, lin.astype(np.float64) + e * d, mel, tgt, h.coeff, prioritize, sr, F)
    # add_loss rounds its inputs to float32: grid values stepped by multiples of 2^-12 survive that rounding exactly
    e = 2.0 ** -10
    d = np.round(d * 4) / 4
    fd = (f(+e)[0] - f(-e)[0]) / (2 * e)
    assert abs(fd - float((got * d).sum())) <= 1e-9 * abs(fd), (fd, float((got * d).sum()))


NEW_SYMBOLS = ("twv_tacotron_cbhg_grad_create", "twv_tacotron_cbhg_grad_destroy", "twv_tacotron_cbhg_grad_workspace_bytes",
               "twv_tacotron_cbhg_grad_route", "twv_tacotron_encoder_grad_run", "twv_tacotron_postnet_grad_run",
               "twv_tacotron_cbhg_grad_set_timing", "twv_tacotron_cbhg_grad_phase_ms", "twv_tacotron_linear_loss_grad")


def test_symbols_are_exported_and_declared():
    import os
    import subprocess
    from twvk_amd import _lib
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "twv_amd.h")).read()
    L = _lib.lib()
    nm = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    for name in NEW_SYMBOLS:
        assert name in _lib.EXPORTS and hasattr(L, name) and name + "(" in header and (" T " + name + "\n") in nm, name
    for kernel in ("cg_gru_forward_kernel", "cg_gru_backward_kernel", "grad_rows_kernel", "cg_bn_bwd_kernel", "cg_highway_bwd_kernel"):
        assert kernel in nm, "the gfx950 kernel %s must be in the library" % kernel


def _create(m, which=0, batch=3, t=19, h="model", out=True):
    from twvk_amd import _lib
    g = C.c_void_p()
    _lib.check(m._L.twv_tacotron_cbhg_grad_create(m._h if h == "model" else None, which, batch, t, C.byref(g) if out else None))
    return g


@pytest.mark.parametrize("kw, message", [
    (dict(h=None), "null argument"), (dict(out=False), "null argument"), (dict(which=2), "which must be"), (dict(which=-1), "which must be"),
    (dict(batch=0), "batch >= 1"), (dict(t=0), "1 <= t_in <= 1024"), (dict(t=1025), "1 <= t_in <= 1024"),
    (dict(which=1, t=0), "1 <= t_out <= max_iters"), (dict(which=1, t=MAX_ITERS * 5 + 1), "1 <= t_out <= max_iters"),
])
def test_create_refuses_invalid_arguments(model, kw, message):
    from twvk_amd._lib import TwvError
    with pytest.raises(TwvError, match="twv_amd error 1: .*" + message):
        _create(model, **kw)


@pytest.mark.parametrize("kw, speakers, message", [(dict(model_type="simple"), 4, "model_type 'simple'"), (dict(enc_proj_width=17), 2, "proj_width above 16"),
                                                   (dict(post_proj_width=17), 2, "proj_width above 16")])
def test_create_refuses_what_is_not_built(kw, speakers, message):
    from twvk_amd._lib import TwvError
    m = _model(num_speakers=speakers, **kw)
    for which in (0, 1):
        if "proj_width" in message and which != ("post_proj_width" in kw):
            m._L.twv_tacotron_cbhg_grad_destroy(_create(m, which, 3, 5))
            continue
        with pytest.raises(TwvError, match="twv_amd error 2: .*" + message + ".*single-speaker and 'deepvoice' models.*projection widths up to 16"):
            _create(m, which, 3, 5)


@pytest.mark.parametrize("kw, speakers", [({}, 2), ({}, 1), (dict(speaker_embedding_size=1), 2), (dict(attention_type="luong"), 2),
                                          (dict(enc_bank_size=16, post_bank_size=1, enc_highway_depth=8, post_highway_depth=1), 2),
                                          (dict(enc_bank_channel_size=30, post_bank_channel_size=30), 2)])
def test_create_accepts_and_labels_its_route(kw, speakers):
    m = _model(num_speakers=speakers, **kw)
    for which, side, t in ((0, "encoder", 19), (1, "post", 40)):
        g = _create(m, which, 3, t)
        try:
            route = dict(kv.split("=", 1) for kv in m._L.twv_tacotron_cbhg_grad_route(g).decode().split())
            assert route["kernel"] == "cg_bigru" and route["side"] == side and route["workgroups_per_utterance"] == "2" and route["weights"] == "registers"
            assert route["bank"] == str(kw.get(("post" if which else "enc") + "_bank_size", 3 if which else 4)) and route["dense"] == str(which)
            assert int(route["lds"]) <= 64 * 1024
            ws = m._L.twv_tacotron_cbhg_grad_workspace_bytes(g)
            g2 = _create(m, which, 3, t - 1)
            assert ws > m._L.twv_tacotron_cbhg_grad_workspace_bytes(g2) > 0
            m._L.twv_tacotron_cbhg_grad_destroy(g2)
        finally:
            m._L.twv_tacotron_cbhg_grad_destroy(g)


ENC_ARGS = ("g", "blob", "tokens", "lengths", "before_highway", "rnn_init", "mask1", "mask2", "d_memory", "workspace", "status", "stream",
            "memory_out", "grad_blob", "d_before_highway", "d_rnn_init")
POST_ARGS = ("g", "blob", "mel", "d_linear", "workspace", "status", "stream", "linear_out", "grad_blob", "d_mel")
ENC_OPTIONAL = ("before_highway", "rnn_init", "mask1", "mask2", "stream", "d_before_highway", "d_rnn_init")


def _args(names, g, null, optional):
    buf = (C.c_float * 16)()
    p = C.cast(buf, C.c_void_p)
    return [None if n in (null,) + tuple(optional) else (g if n == "g" else p) for n in names], p


@pytest.mark.parametrize("null", [a for a in ENC_ARGS if a not in ENC_OPTIONAL])
def test_encoder_run_refuses_null_arguments(model, null):
    from twvk_amd import _lib
    g = _create(model)
    try:
        with pytest.raises(_lib.TwvError, match="twv_amd error 1: null argument"):
            _lib.check(model._L.twv_tacotron_encoder_grad_run(*_args(ENC_ARGS, g, null, ENC_OPTIONAL)[0]))
    finally:
        model._L.twv_tacotron_cbhg_grad_destroy(g)


@pytest.mark.parametrize("null", [a for a in POST_ARGS if a != "stream"])
def test_postnet_run_refuses_null_arguments(model, null):
    from twvk_amd import _lib
    g = _create(model, 1, 3, 40)
    try:
        with pytest.raises(_lib.TwvError, match="twv_amd error 1: null argument"):
            _lib.check(model._L.twv_tacotron_postnet_grad_run(*_args(POST_ARGS, g, null, ("stream",))[0]))
    finally:
        model._L.twv_tacotron_cbhg_grad_destroy(g)


def test_runs_refuse_the_other_side_and_inputs_without_their_outputs(model):
    from twvk_amd import _lib
    ge, gp = _create(model), _create(model, 1, 3, 40)
    try:
        a, p = _args(ENC_ARGS, gp, None, ENC_OPTIONAL)
        with pytest.raises(_lib.TwvError, match="twv_amd error 1: the handle was created for the post net"):
            _lib.check(model._L.twv_tacotron_encoder_grad_run(*a))
        with pytest.raises(_lib.TwvError, match="twv_amd error 1: the handle was created for the encoder"):
            _lib.check(model._L.twv_tacotron_postnet_grad_run(*_args(POST_ARGS, ge, None, ("stream",))[0]))
        for given in ("before_highway", "rnn_init"):
            a, p = _args(ENC_ARGS, ge, None, ENC_OPTIONAL)
            a[ENC_ARGS.index(given)] = p
            with pytest.raises(_lib.TwvError, match="twv_amd error 1: null argument: before_highway / rnn_init need their d_ outputs"):
                _lib.check(model._L.twv_tacotron_encoder_grad_run(*a))
        ms = (C.c_double * 4)()
        _lib.check(model._L.twv_tacotron_cbhg_grad_set_timing(ge, 1))
        with pytest.raises(_lib.TwvError, match="twv_amd error 1: no run with timing on"):
            _lib.check(model._L.twv_tacotron_cbhg_grad_phase_ms(ge, ms))
        with pytest.raises(_lib.TwvError, match="twv_amd error 1: null argument"):
            _lib.check(model._L.twv_tacotron_cbhg_grad_phase_ms(ge, None))
    finally:
        model._L.twv_tacotron_cbhg_grad_destroy(ge)
        model._L.twv_tacotron_cbhg_grad_destroy(gp)


@pytest.mark.parametrize("null", ["linear", "linear_targets", "coeff", "d_linear"])
def test_linear_loss_grad_refuses_null_arguments(model, null):
    from twvk_amd import _lib
    buf = (C.c_float * 16)()
    p = C.cast(buf, C.c_void_p)
    a = {n: (None if n == null else p) for n in ("linear", "linear_targets", "coeff", "d_linear")}
    with pytest.raises(_lib.TwvError, match="twv_amd error 1: null argument"):
        _lib.check(model._L.twv_tacotron_linear_loss_grad(a["linear"], a["linear_targets"], a["coeff"], 3, 25, 129, 0, 24000.0, a["d_linear"], None))
    with pytest.raises(_lib.TwvError, match="twv_amd error 1: batch, t_out and num_freq"):
        _lib.check(model._L.twv_tacotron_linear_loss_grad(p, p, p, 3, 0, 129, 0, 24000.0, p, None))
    with pytest.raises(_lib.TwvError, match="twv_amd error 1: prioritize_loss needs sample_rate > 0"):
        _lib.check(model._L.twv_tacotron_linear_loss_grad(p, p, p, 3, 5, 129, 1, 0.0, p, None))


def test_python_methods_refuse_without_a_teacher_forced_pass(model):
    for call in (lambda: model.linear_loss_cotangent(np.zeros((3, 25, 129), np.float32)), lambda: model.postnet_grad(np.zeros((3, 25, 129), np.float32)),
                 lambda: model.encoder_grad(np.zeros((3, 19, 256), np.float32)), lambda: model.loss_gradients(np.zeros((3, 25, 129), np.float32))):
        with pytest.raises(ValueError, match="teacher_forced=True"):
            call()


def test_grad_layouts_cover_their_tensors():
    from twvk_amd.tacotron import decoder_grad_layout, encoder_grad_layout, flatten, postnet_grad_layout
    import torch_tacotron_cbhg_grad_ref as CG
    h = host_case("A-masked-tails")
    blob = flatten(h.specs, h.w)
    enc, post, dec = encoder_grad_layout(h.specs), postnet_grad_layout(h.specs), decoder_grad_layout(h.specs)
    assert [n for n, _, _ in enc] == h.enc_names and [n for n, _, _ in post] == h.post_names
    assert post[-1][1] + int(np.prod(post[-1][2])) == blob.size and enc[0][1] == 0
    spans = sorted((o, o + int(np.prod(s))) for _, o, s in enc + dec + post)
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))
    for name, off, shp in enc + post:
        if name.endswith("batch_normalization"):
            assert shp == (2, h.w[name].shape[1])
        else:
            assert np.array_equal(blob[off:off + int(np.prod(shp))].reshape(shp), h.w[name]), name
    assert set(CG.model_names(h.specs)) == {n for n, _, _ in enc + dec + post}


def _view(m, batch, t_in, which):
    from twvk_amd import _lib
    off, n = C.c_longlong(-1), C.c_longlong(-1)
    _lib.check(m._L.twv_tacotron_workspace_view(m._h, batch, t_in, which.encode(), C.byref(off), C.byref(n)))
    return off.value, n.value


def test_workspace_bytes_are_unchanged_and_the_new_views_lie_inside():
    import twvk_amd
    from twvk_amd.tacotron import Tacotron
    from twvk_amd._lib import TwvError
    m = Tacotron(twvk_amd.default_hparams(), num_speakers=2)
    got = tuple(int(m._L.twv_tacotron_workspace_bytes(m._h, n, t)) for n, t in WS_CASES)
    assert got == WS_PARENT, got
    hp = m._hparams
    for n, t in WS_CASES:
        total = m._L.twv_tacotron_workspace_bytes(m._h, n, t) // 4
        names = ("memory", "keys", "decoder_init", "before_highway", "encoder_rnn_init")
        pieces = sorted(_view(m, n, t, which) for which in names)
        assert _view(m, n, t, "before_highway")[1] == n * hp.enc_prenet_sizes[1] and _view(m, n, t, "encoder_rnn_init")[1] == n * 2 * hp.enc_rnn_size
        assert pieces[0][0] >= 0 and pieces[-1][0] + pieces[-1][1] <= total
        for (o0, n0), (o1, _) in zip(pieces, pieces[1:]):
            assert o0 + n0 <= o1 and o0 % 4 == 0 and o1 % 4 == 0, (n, t, pieces)
    with pytest.raises(TwvError, match="twv_amd error 1: .*no piece named 'values'"):
        _view(m, 2, 5, "values")
    for m1 in (Tacotron(twvk_amd.default_hparams(), num_speakers=1), _model(num_speakers=4, model_type="simple")):
        for which in ("before_highway", "encoder_rnn_init"):
            with pytest.raises(TwvError, match="twv_amd error 1: .*this model has no '%s'" % which):
                _view(m1, 2, 5, which)
        assert _view(m1, 2, 5, "memory")[1] == 2 * 5 * 2 * hp.enc_rnn_size
    ms = _model(speaker_embedding_size=1)
    assert _view(ms, 2, 5, "before_highway")[1] == 2 * hp.enc_prenet_sizes[1]
