"""Generation at residual / dilation widths 64 and 128 (wn_wide_generate_kernel), bit for bit against the CPU oracle through the C-ABI.

Input condition (so that sample equality cannot hide a wrong network): the MoL sampler clamps to +-1, and with plain random weights
about half of the oracle's samples sit on the clamp.  Every MoL case that has biases therefore builds its weights with scale 0.05
and lowers the log-scale third of wavenet/conv1d_2/bias by 5, and asserts on the ORACLE's output, before comparing, that at most 5 %
of the samples are +-1.  The cases that go through run_mol / run_onehot also put every mixture selection / every one-hot draw on its
edge (tests/sensitive_inputs.py: knife_edge_mol, knife_edge_onehot; use_bias=False variants get the narrowed logistic draw
instead of the shift) and assert the edge count and the uniform range.  Exempt: the layer-dump cases (plain inputs; the MoL one at scale 0.2, the one-hot ones at 0.3: the dumps
compare z, x and the raw outputs directly -- the peaked one-hot distribution of scale 0.3 is covered there and nowhere else),
test_wide_keeps_the_clamp_covered (plain inputs on purpose), and test_wide_generate_cli_restores_a_bundle, whose uniforms are drawn
by the command line tool from its --seed and cannot be injected: shifted head, clamp share asserted."""
import json

import numpy as np
import pytest

from helpers import first_mismatch, mol_uniforms, sensitive_mol, sensitive_onehot
from sensitive_inputs import assert_off_the_clamp, shift_mol_head

pytestmark = pytest.mark.gpu

WIDTHS = [(64, 64), (128, 128), (32, 64), (64, 32), (128, 64)]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def make_case(O, dilations, R, D, scalar_input=True, S=512, Q=256, out_channels=30, ifw=32, use_bias=True, G=32, gc_card=2, L=80,
              up=(5, 5, 12), seed=0, scale=0.05, shift=True):
    d = O.make_dims(dilations, R=R, D=D, S=S, Q=Q, out_channels=out_channels, scalar_input=scalar_input, ifw=ifw, use_bias=use_bias,
                    G=G, gc_card=gc_card, L=L, up=up)
    tensors = dict(O.random_tensors(d, seed=seed, scale=scale))
    if shift and scalar_input:
        tensors = shift_mol_head(tensors, out_channels)      # narrow mixture components: the samples leave the clamp
    return d, tensors, O.blob_from_tensors(d, tensors)


def make_model(batch, dilations, tensors, R, D, scalar_input=True, S=512, Q=256, out_channels=30, ifw=32, use_bias=True, G=32, gc_card=2,
               L=80, up=(5, 5, 12), options=()):
    import twvk_amd  # noqa: F401
    from twvk_amd.wavenet import WaveNetModel
    m = WaveNetModel(batch, dilations, 2, R, D, S, quantization_channels=Q, out_channels=out_channels, use_biases=use_bias,
                     scalar_input=scalar_input, initial_filter_width=ifw, global_condition_channels=G or None,
                     global_condition_cardinality=(gc_card or None) if G else None, local_condition_channels=L or None,
                     upsample_factor=list(up) if L else None, train_mode=False)
    for k, v in options:
        m.set_option(k, v)
    m.load_weights(tensors)
    return m


def run_mol(O, dil, B, R, D, T=None, t_mel=1, debug_steps=0, options=(), seed=0, scale=0.05, shift=True, **kw):
    d, tensors, blob = make_case(O, dil, R, D, seed=seed, scale=scale, shift=shift, **kw)
    m = make_model(B, dil, tensors, R, D, options=options, **kw)
    rng = np.random.RandomState(1)
    G, L = kw.get("G", 32), kw.get("L", 80)
    if L:
        hop = int(np.prod(kw.get("up", (5, 5, 12))))
        if T is None:
            T = t_mel * hop
        mel = rng.uniform(-4, 4, (B, (T + hop - 1) // hop, L)).astype(np.float32)
        U_o = O.upsample(d, blob, mel)[:, :T].copy()
        U_g = m.create_upsample(mel)[:, :T].contiguous()
    else:
        T = T or 300
        U_o = U_g = None
    gc = (np.arange(B) % 2).astype(np.int32) if G else None
    seed_in = (2 * rng.rand(B) - 1).astype(np.float32)
    if shift:
        u, want = sensitive_mol(O, d, blob, U_o, gc, seed_in, B, T)
    else:
        u = mol_uniforms(B, T, d.O // 3)
        want = O.generate_mol(d, blob, O.State(d, B), U_o, gc, seed_in, u)
    res = m.generate(U_g, gc, seed_in, u, debug_steps=debug_steps)
    return d, blob, m, want, res, (U_o, U_g, gc, seed_in, u)


def run_onehot(O, dil, B, T, R, D, temperature=1.0, debug_steps=0, scale=0.12, sensitive=True, **kw):
    """scale 0.12: at 0.3 the distribution is so peaked that more than 10 % of the draws land in the last non-empty class, where
    no edge exists; the layer-dump cases keep 0.3 and plain draws (sensitive=False)"""
    Q = kw.get("Q", 256)
    d, tensors, blob = make_case(O, dil, R, D, scalar_input=False, scale=scale, **kw)
    m = make_model(B, dil, tensors, R, D, scalar_input=False, **kw)
    rng = np.random.RandomState(7)
    L, G = kw.get("L", 80), kw.get("G", 32)
    U = rng.uniform(-4, 4, (B, T, L)).astype(np.float32) if L else None
    gc = (np.arange(B) % 2).astype(np.int32) if G else None
    seed_in = rng.randint(Q, size=B).astype(np.int32)
    u = rng.random_sample((B, T))
    if sensitive:
        u, want = sensitive_onehot(O, d, blob, U, gc, seed_in, u, temperature)
    else:
        want = O.generate_mulaw(d, blob, O.State(d, B), U, gc, seed_in, u, temperature)
    res = m.generate(U, gc, seed_in, u, temperature=temperature, debug_steps=debug_steps)
    return d, blob, m, want, res, (U, gc, seed_in, u)


def check_dumps(O, d, blob, dump, want, seed_in, U, gc, B, NL, dbg):
    R, D = d.R, d.D
    st = O.State(d, B)
    inp = seed_in.copy()
    for t in range(dbg):
        raw, dz, dx = O.step(d, blob, st, inp, U[:, t], gc, debug=True)
        lay = dump[:, t, :NL * (D + R)].reshape(B, NL, D + R)
        assert first_mismatch(lay[:, :, :D], dz) is None, ("z", t, first_mismatch(lay[:, :, :D], dz))
        assert first_mismatch(lay[:, :, D:], dx) is None, ("x", t, first_mismatch(lay[:, :, D:], dx))
        graw = dump[:, t, NL * (D + R):NL * (D + R) + d.O]
        assert first_mismatch(graw, raw) is None, ("raw", t, first_mismatch(graw, raw))
        inp = want[:, t]


# ---------------------------------------------------------------- 1. layer dumps
@pytest.mark.parametrize("R,D", WIDTHS)
def test_wide_layer_dumps(torch_cuda, oracle, R, D):
    """first line of defence: per-layer z (D) / x (R) and the raw outputs of the first steps against the oracle's own dumps"""
    dil = [1, 2, 4, 8, 1, 2, 4, 8]
    B, T, dbg = 2, 24, 4
    d, blob, m, want, (got, dump), (U_o, _, gc, seed_in, u) = run_mol(oracle, dil, B, R, D, T=T, debug_steps=dbg, scale=0.2, shift=False)
    assert m.kernel_name() == "wn_wide_generate_kernel" and not m.fused_conditioning()
    check_dumps(oracle, d, blob, dump.cpu().numpy(), want, seed_in, U_o, gc, B, len(dil), dbg)
    assert first_mismatch(got.cpu().numpy(), want) is None


@pytest.mark.parametrize("temperature", [1.0, 0.8])
@pytest.mark.parametrize("R,D", [(64, 64), (128, 128)])
def test_wide_onehot_layer_dumps(torch_cuda, oracle, R, D, temperature):
    dil = [1, 2, 4, 8, 1, 2, 4, 8]
    B, T, dbg = 2, 40, 3
    d, blob, m, want, (got, dump), (U, gc, seed_in, u) = run_onehot(oracle, dil, B, T, R, D, S=128, temperature=temperature, debug_steps=dbg,
                                                                            scale=0.3, sensitive=False)
    check_dumps(oracle, d, blob, dump.cpu().numpy(), want, seed_in, U, gc, B, len(dil), dbg)
    assert np.array_equal(got.cpu().numpy(), want), first_mismatch(got.cpu().numpy(), want)


# ---------------------------------------------------------------- 2. variants
VARIANT_DIL = [1, 2, 4, 8, 16, 1, 2]


def test_wide_keeps_the_clamp_covered(torch_cuda, oracle):
    """the sampler's clamp to +-1 stays tested: plain inputs ON PURPOSE (unshifted head at scale 0.1, plain uniforms); the oracle's
    samples must hold +1, -1 and values strictly inside"""
    d, blob, m, want, got, _ = run_mol(oracle, VARIANT_DIL, 3, 64, 64, T=70, scale=0.1, shift=False)
    assert (want == 1.0).any() and (want == -1.0).any() and (np.abs(want) < 1.0).any()
    assert first_mismatch(got.cpu().numpy(), want) is None


@pytest.mark.parametrize("kw", [dict(), dict(use_bias=False), dict(G=0), dict(L=0), dict(ifw=8), dict(S=64), dict(S=1024), dict(up=(3, 4))])
def test_wide_variants_64(torch_cuda, oracle, kw):
    d, blob, m, want, got, _ = run_mol(oracle, VARIANT_DIL, 3, 64, 64, T=70, **kw)
    assert first_mismatch(got.cpu().numpy(), want) is None, kw


@pytest.mark.parametrize("R,D", [(128, 128), (32, 128)])
@pytest.mark.parametrize("kw", [dict(), dict(use_bias=False, G=0, L=0)])
def test_wide_variants_other_widths(torch_cuda, oracle, R, D, kw):
    d, blob, m, want, got, _ = run_mol(oracle, VARIANT_DIL, 3, R, D, T=70, **kw)
    assert first_mismatch(got.cpu().numpy(), want) is None, (R, D, kw)


def test_wide_global_condition_passed_as_embedding(torch_cuda, oracle):
    """model.py:199-207: no cardinality, the caller passes the (B, gc_channels) embedding itself"""
    dil, B, T = VARIANT_DIL, 3, 70
    d_id, tensors_id, blob_id = make_case(oracle, dil, 64, 64, gc_card=3, seed=4)
    table = tensors_id["wavenet/gc_embedding"]
    ids = np.array([2, 0, 1], np.int32)
    rng = np.random.RandomState(6)
    mel = rng.uniform(-4, 4, (B, 1, 80)).astype(np.float32)
    seed_in = (2 * rng.rand(B) - 1).astype(np.float32)
    u, want = sensitive_mol(oracle, d_id, blob_id, oracle.upsample(d_id, blob_id, mel)[:, :T].copy(), ids, seed_in, B, T)
    tensors_e = {k: v for k, v in tensors_id.items() if k != "wavenet/gc_embedding"}
    m = make_model(B, dil, tensors_e, 64, 64, gc_card=0)
    got = m.generate(m.create_upsample(mel)[:, :T].contiguous(), table[ids], seed_in, u).cpu().numpy()
    assert first_mismatch(got, want) is None, first_mismatch(got, want)


@pytest.mark.parametrize("kw", [dict(Q=256), dict(Q=64), dict(Q=16, L=0, G=0)])
def test_wide_onehot_variants(torch_cuda, oracle, kw):
    d, blob, m, want, got, _ = run_onehot(oracle, VARIANT_DIL, 3, 70, 64, 64, S=128, **kw)
    assert np.array_equal(got.cpu().numpy(), want), (kw, first_mismatch(got.cpu().numpy(), want))


# ---------------------------------------------------------------- 3. C2 stack
@pytest.mark.parametrize("R,D,B", [(64, 64, 2), (128, 128, 2), (64, 64, 8)])
def test_wide_c2_stack(torch_cuda, oracle, R, D, B):
    """C2 architecture (3 x [1..512], S = 512, MoL-30, gc + lc), 2 mel frames = 600 samples; B = 8 is the geometry of the measurement"""
    dil = [2 ** i for i in range(10)] * 3
    d, blob, m, want, got, _ = run_mol(oracle, dil, B, R, D, t_mel=2)
    got = got.cpu().numpy()
    assert got.shape == want.shape == (B, 600)
    assert first_mismatch(got, want) is None, first_mismatch(got, want)


def test_wide_c2_stack_onehot_draws_many_classes(torch_cuda, oracle):
    dil = [2 ** i for i in range(10)] * 3
    d, blob, m, want, got, _ = run_onehot(oracle, dil, 2, 600, 64, 64)
    assert len(np.unique(want)) >= 50, len(np.unique(want))
    assert np.array_equal(got.cpu().numpy(), want), first_mismatch(got.cpu().numpy(), want)


# ---------------------------------------------------------------- 4. delay lines wrap
@pytest.mark.parametrize("R,D", [(64, 64), (128, 32)])
def test_wide_past_longest_delay_line(torch_cuda, oracle, R, D):
    """long enough that every delay line (d = 512) wraps more than twice"""
    dil = [1, 4, 16, 64, 256, 512]
    d, blob, m, want, got, _ = run_mol(oracle, dil, 1, R, D, t_mel=5, S=128)
    assert got.shape == (1, 1500)
    assert first_mismatch(got.cpu().numpy(), want) is None


# ---------------------------------------------------------------- 5. state carries over
def test_wide_state_carries_over_mol(torch_cuda, oracle):
    dil = [2 ** i for i in range(8)]
    d, blob, m, want, got, (U_o, U_g, gc, seed_in, u) = run_mol(oracle, dil, 2, 64, 64, t_mel=2)
    assert first_mismatch(got.cpu().numpy(), want) is None
    m.queue_initializer()
    a = m.generate(U_g[:, :250].contiguous(), gc, seed_in, u[:, :250]).cpu().numpy()
    b = m.generate(U_g[:, 250:].contiguous(), gc, a[:, -1], u[:, 250:]).cpu().numpy()
    assert first_mismatch(np.concatenate([a, b], axis=1), want) is None


def test_wide_state_carries_over_onehot(torch_cuda, oracle):
    dil = [2 ** i for i in range(8)]
    d, blob, m, want, got, (U, gc, seed_in, u) = run_onehot(oracle, dil, 2, 600, 64, 64, S=128)
    assert len(np.unique(want)) >= 50
    assert np.array_equal(got.cpu().numpy(), want)
    m.queue_initializer()
    a = m.generate(U[:, :250], gc, seed_in, u[:, :250]).cpu().numpy()
    b = m.generate(U[:, 250:], gc, a[:, -1], u[:, 250:]).cpu().numpy()
    assert np.array_equal(np.concatenate([a, b], axis=1), want)


# ---------------------------------------------------------------- 6. priming then generation
@pytest.mark.parametrize("scalar", [True, False])
@pytest.mark.parametrize("R,D", [(64, 64), (128, 128)])
def test_wide_priming_then_generation(torch_cuda, oracle, R, D, scalar):
    """generate.py:168-180: prime with RF-1 seed samples (zero lc, predictions discarded), then generate"""
    dil = [1, 2, 4, 8, 16]
    B, T = 2, 30
    d, tensors, blob = make_case(oracle, dil, R, D, scalar_input=scalar, S=128, Q=64, scale=0.05 if scalar else 0.25)
    m = make_model(B, dil, tensors, R, D, scalar_input=scalar, S=128, Q=64)
    rf = oracle.receptive_field(d)
    assert m.receptive_field == rf
    rng = np.random.RandomState(9)
    seedwave = rng.uniform(-1, 1, (B, rf)).astype(np.float32) if scalar else rng.randint(64, size=(B, rf)).astype(np.int32)
    U = rng.uniform(-4, 4, (B, T, 80)).astype(np.float32)
    gc = np.array([0, 1], np.int32)
    if scalar:
        u, want = sensitive_mol(oracle, d, blob, U, gc, seedwave[:, -1], B, T, prime=seedwave[:, :rf - 1])
    else:
        u, want = sensitive_onehot(oracle, d, blob, U, gc, seedwave[:, -1], np.random.RandomState(3).random_sample((B, T)), 1.0,
                                   prime=seedwave[:, :rf - 1])
    m.prime(seedwave[:, :rf - 1], None, gc)
    got = m.generate(U, gc, seedwave[:, -1], u).cpu().numpy()
    assert first_mismatch(got, want) is None


# ---------------------------------------------------------------- 7. batch and lengths
@pytest.mark.parametrize("B", [1, 300])
def test_wide_batch(torch_cuda, oracle, B):
    """B = 300 is more streams than the device has CUs: legal, the workgroups of the wide kernel do not wait for each other"""
    d, blob, m, want, got, _ = run_mol(oracle, [1, 2, 4], B, 64, 64, T=12, S=64)
    assert first_mismatch(got.cpu().numpy(), want) is None


@pytest.mark.parametrize("T", [1, 3, 37])
def test_wide_single_step_and_ragged_lengths(torch_cuda, oracle, T):
    d, blob, m, want, got, _ = run_mol(oracle, [1, 2, 4, 8], 2, 64, 64, T=T, S=64)
    assert got.shape == (2, T)
    assert first_mismatch(got.cpu().numpy(), want) is None, T


# ---------------------------------------------------------------- 8. bounded conditioning table
def test_wide_conditioning_is_bounded(torch_cuda, oracle):
    dil = [1, 2, 4, 8, 16]
    B, T, R, D = 2, 900, 64, 64
    d, tensors, blob = make_case(oracle, dil, R, D, S=128)
    rng = np.random.RandomState(2)
    mel = rng.uniform(-4, 4, (B, 3, 80)).astype(np.float32)
    gc = np.array([0, 1], np.int32)
    seed_in = (2 * rng.rand(B) - 1).astype(np.float32)
    u, want = sensitive_mol(oracle, d, blob, oracle.upsample(d, blob, mel), gc, seed_in, B, T)
    m = make_model(B, dil, tensors, R, D, S=128)
    m.MAX_COND_BYTES = 4 * B * len(dil) * 2 * D * 450         # room for 450 steps -> one hop (300 steps) per call: three calls
    assert m._steps_per_call(T) == 300
    got = m.generate(m.create_upsample(mel), gc, seed_in, u).cpu().numpy()
    assert first_mismatch(got, want) is None, first_mismatch(got, want)


# ---------------------------------------------------------------- 9. predict_proba_incremental
def test_wide_predict_proba_incremental_returns_probabilities(torch_cuda, oracle):
    """model.py:241-243: tf.cast(softmax(float64(logits)), float32), (B, Q); tolerance 1e-6 on probabilities as in the test of the
    same name at width 32"""
    dil = [1, 2, 4, 8, 1, 2]
    B, Q, R, D = 2, 256, 64, 128
    d, tensors, blob = make_case(oracle, dil, R, D, scalar_input=False, S=128, Q=Q, scale=0.3)
    m = make_model(B, dil, tensors, R, D, scalar_input=False, S=128, Q=Q)
    rng = np.random.RandomState(5)
    U = rng.uniform(-4, 4, (B, 3, 80)).astype(np.float32)
    gc = np.array([1, 0], np.int32)
    st = oracle.State(d, B)
    inp = rng.randint(Q, size=B).astype(np.int32)
    for t in range(3):
        raw, _, _ = oracle.step(d, blob, st, inp, U[:, t], gc, debug=True)
        x = raw.astype(np.float64)
        e = np.exp(x - x.max(axis=1, keepdims=True))
        want = (e / e.sum(axis=1, keepdims=True)).astype(np.float32)
        got = m.predict_proba_incremental(inp, U[:, t], gc).cpu().numpy()
        assert got.shape == (B, Q) and got.dtype == np.float32
        assert np.abs(got - want).max() <= 1e-6, (t, np.abs(got - want).max())
        assert abs(float(got.sum(axis=1).max()) - 1.0) < 1e-5
        inp = want.argmax(axis=1).astype(np.int32)


# ---------------------------------------------------------------- 10. CLI + TF bundle
def test_wide_generate_cli_restores_a_bundle(torch_cuda, oracle, tmp_path):
    """params.json carries the widths; the wave is ops.wav_to_int16 of the oracle's samples for the same seed"""
    from scipy.io import wavfile
    import twvk_amd
    from twvk_amd import checkpoint as ck, ops
    from twvk_amd.generate import main
    logdir = tmp_path / "ckpt"; logdir.mkdir()
    dil = [1, 2, 4, 8, 16, 32]
    json.dump({"dilations": dil, "skip_channels": 128, "residual_channels": 64, "dilation_channels": 64}, open(logdir / "params.json", "w"))
    d, tensors, blob = make_case(oracle, dil, 64, 64, S=128, seed=11)
    var = dict(tensors)
    var["global_step"] = np.asarray(5, np.int32)
    ck.write_bundle(str(logdir / "model.ckpt-5"), var)
    ck.write_checkpoint_state(str(logdir), str(logdir / "model.ckpt-5"))
    mel = np.random.RandomState(0).uniform(-4, 4, (2, 80)).astype(np.float32)
    np.save(tmp_path / "mel.npy", mel)
    try:
        paths = main([str(logdir), "--mel", str(tmp_path / "mel.npy"), "--gc_cardinality", "2", "--gc_id", "1", "--batch_size", "1",
                      "--seed", "3", "--logdir", str(tmp_path / "log")])
        rate, data = wavfile.read(paths[0])
    finally:
        twvk_amd.hparams.__dict__.update(twvk_amd.default_hparams().__dict__)
    rng = np.random.RandomState(3)                                      # generate.py's draws for --seed 3
    first = (2 * rng.rand(1) - 1).astype(np.float32)
    lo, hi = np.float32(1e-5), np.float32(1. - 1e-5)
    u = (rng.random_sample((1, 600, 11)).astype(np.float32) * (hi - lo) + lo).astype(np.float32)
    want = oracle.generate_mol(d, blob, oracle.State(d, 1), oracle.upsample(d, blob, mel[None]), np.array([1], np.int32), first, u)
    assert_off_the_clamp(want)
    want16 = ops.wav_to_int16(torch_cuda.as_tensor(want, device="cuda")).cpu().numpy()
    assert data.shape == (600,) and np.array_equal(data, want16[0])


# ---------------------------------------------------------------- 11. options are inert
def test_wide_launch_geometry_options_are_inert(torch_cuda, oracle):
    d, blob, m, want, got, _ = run_mol(oracle, VARIANT_DIL, 3, 64, 64, T=70, options=(("groups", 2), ("xcd", 0), ("helpers", 0)))
    assert m.kernel_name() == "wn_wide_generate_kernel"
    assert first_mismatch(got.cpu().numpy(), want) is None


# ---------------------------------------------------------------- 12. the reported error path
def test_wide_nan_logits_are_an_error_not_a_sample(torch_cuda, oracle):
    from twvk_amd._lib import TwvError
    dil = [1, 2, 4, 8]
    d, tensors, blob = make_case(oracle, dil, 64, 64, scalar_input=False, Q=256)
    b2 = tensors["wavenet/conv1d_2/bias"].copy(); b2[17] = np.nan
    tensors["wavenet/conv1d_2/bias"] = b2
    m = make_model(2, dil, tensors, 64, 64, scalar_input=False, Q=256)
    rng = np.random.RandomState(5)
    with pytest.raises(TwvError, match="NaN"):
        m.generate(rng.uniform(-4, 4, (2, 40, 80)).astype(np.float32), np.array([0, 1], np.int32), np.array([128, 3], np.int32),
                   rng.random_sample((2, 40)))
