"""-m gpu: the chain workgroup's relay of SIX waves with FIVE layers each (wn_xcd_generate_kernel; the head wave carries the causal
layer and the sampler only), bit for bit against the CPU oracle.

What can go wrong with the layer-to-wave map shows at its edges: a stack that ends inside a wave's block of five, exactly at its end
or one layer past it (the wave's first layer, its count, "a later wave continues the stack", the deferred granule stores of the waves
that are not last, the immediate ones of the last), the teacher-forced instantiation, the hand-off to the second chain workgroup
behind layer 30 and the blocks of five there, and the one-hot model on the same template.  Inputs as in tests/test_wavenet_gpu.py
(tests/sensitive_inputs.py): shifted head, every selection on its edge, conditions asserted on the oracle's output."""
import numpy as np
import pytest

from helpers import first_mismatch, make_case, make_model, mol_uniforms, sensitive_mol, sensitive_onehot

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def _dil7(nl):
    return ([1, 2, 4, 8, 16, 32, 64] * 5)[:nl]


def _dil10(nl):
    return ([2 ** i for i in range(10)] * 5)[:nl]


_cases = {}


def _mol_case(oracle, nl, B, T, use_bias=True, G=32, L=80, dil=None, frames=2):
    """(d, blob, tensors, dil, mel, gc, seed_in, u, want), built once per shape and shared (nobody writes to it)"""
    key = (nl, B, T, use_bias, G, L, None if dil is None else tuple(dil), frames)
    if key not in _cases:
        dil_ = list(dil) if dil is not None else _dil7(nl)
        d, tensors, blob = make_case(oracle, dil_, use_bias=use_bias, G=G, L=L, shift=5.0)
        rng = np.random.RandomState(nl)
        mel = rng.uniform(-4, 4, (B, frames, 80)).astype(np.float32) if L else None
        gc = (np.arange(B) % 2).astype(np.int32) if G else None
        seed_in = (2 * rng.rand(B) - 1).astype(np.float32)
        u, want = sensitive_mol(oracle, d, blob, oracle.upsample(d, blob, mel)[:, :T] if L else None, gc, seed_in, B, T)
        _cases[key] = (d, blob, tensors, dil_, mel, gc, seed_in, u, want)
    return _cases[key]


@pytest.mark.parametrize("nl,kw", [(4, {}), (5, {}), (6, {}), (10, {}), (11, {}), (26, {}), (29, {}), (30, {}),
                                   (6, dict(use_bias=False, G=0, L=0)), (26, dict(use_bias=False, G=0, L=0))])
def test_layer_counts_at_the_wave_edges(torch_cuda, oracle, nl, kw):
    """a last wave of 4, 5, 1 (behind one or two full waves), 1 and 4 (behind five) and 5 layers: the smallest shapes at which a wrong
    first layer, layer count, next-wave flag or deferred-store rule of a wave changes a sample"""
    B, T = 3, 450
    d, blob, tensors, dil, mel, gc, seed_in, u, want = _mol_case(oracle, nl, B, T, **kw)
    use_bias, G, L = kw.get("use_bias", True), kw.get("G", 32), kw.get("L", 80)
    m = make_model(B, dil, tensors, use_bias=use_bias, G=G, L=L)
    assert m.fused_conditioning() == bool(L)
    got = m.generate(m.create_upsample(mel) if L else None, gc, seed_in, u).cpu().numpy()
    assert first_mismatch(got, want) is None, first_mismatch(got, want)


def test_layer_dumps_across_three_waves(torch_cuda, oracle):
    """z and the layer input of every one of 11 layers (waves 0, 1 and the single layer of wave 2) and the raw outputs of the first steps
    against the oracle's own dumps: a layer served by the wrong wave or tile shows here directly, not through the sampler.  Plain
    inputs at scale 0.2, as tests/test_wavenet_gpu.py::test_generate_small_with_layer_dumps"""
    nl, B, T, dbg = 11, 2, 24, 4
    dil = _dil7(nl)
    d, tensors, blob = make_case(oracle, dil, scale=0.2)
    m = make_model(B, dil, tensors)
    assert m.fused_conditioning()
    rng = np.random.RandomState(1)
    mel = rng.uniform(-4, 4, (B, 1, 80)).astype(np.float32)
    U_o = oracle.upsample(d, blob, mel)[:, :T]
    gc = (np.arange(B) % 2).astype(np.int32)
    seed_in = (2 * rng.rand(B) - 1).astype(np.float32)
    u = mol_uniforms(B, T, d.O // 3)
    want = oracle.generate_mol(d, blob, oracle.State(d, B), U_o, gc, seed_in, u)
    got, dump = m.generate(m.create_upsample(mel)[:, :T].contiguous(), gc, seed_in, u, debug_steps=dbg)
    dump = dump.cpu().numpy()
    st = oracle.State(d, B)
    inp = seed_in.copy()
    for t in range(dbg):
        raw, dz, dx = oracle.step(d, blob, st, inp, U_o[:, t], gc, debug=True)
        gz = dump[:, t, :nl * 64].reshape(B, nl, 2, 32)
        assert first_mismatch(gz[:, :, 0], dz) is None, ("z", t, first_mismatch(gz[:, :, 0], dz))
        assert first_mismatch(gz[:, :, 1], dx) is None, ("x", t, first_mismatch(gz[:, :, 1], dx))
        graw = dump[:, t, nl * 64:nl * 64 + d.O]
        assert first_mismatch(graw, raw) is None, ("raw", t, first_mismatch(graw, raw))
        inp = want[:, t]
    assert first_mismatch(got.cpu().numpy(), want) is None


def _primed(torch_cuda, oracle, dil, B, T):
    d, tensors, blob = make_case(oracle, dil, shift=5.0)
    m = make_model(B, dil, tensors)
    assert m.fused_conditioning()
    rf = oracle.receptive_field(d)
    rng = np.random.RandomState(9)
    seedwave = rng.uniform(-1, 1, (B, rf)).astype(np.float32)
    mel = rng.uniform(-4, 4, (B, 1, 80)).astype(np.float32)
    gc = (np.arange(B) % 2).astype(np.int32)
    u, want = sensitive_mol(oracle, d, blob, oracle.upsample(d, blob, mel)[:, :T], gc, seedwave[:, -1], B, T, prime=seedwave[:, :rf - 1])
    m.prime(seedwave[:, :rf - 1], None, gc)
    got = m.generate(m.create_upsample(mel)[:, :T].contiguous(), gc, seedwave[:, -1], u).cpu().numpy()
    assert first_mismatch(got, want) is None, first_mismatch(got, want)


def test_teacher_forced_steps_with_a_five_layer_wave(torch_cuda, oracle):
    """generate.py:168-180: RF-1 teacher-forced samples through waves of 5, 5 and 1 layers (the run-time-count instantiation; the last
    layer's wave reports the end of a step to the head), then generation from the primed queues"""
    _primed(torch_cuda, oracle, _dil7(11), 3, 300)


def test_chunked_calls(torch_cuda, oracle):
    """300 + 150 steps in two calls equal the 450 of one (the second call's seed is the first's last sample): the state a call leaves
    does not depend on which wave ran a layer"""
    nl, B, T = 30, 3, 450
    d, blob, tensors, dil, mel, gc, seed_in, u, want = _mol_case(oracle, nl, B, T)
    m = make_model(B, dil, tensors)
    U = m.create_upsample(mel)
    a = m.generate(U[:, :300].contiguous(), gc, seed_in, u[:, :300]).cpu().numpy()
    b = m.generate(U[:, 300:450].contiguous(), gc, a[:, -1], u[:, 300:]).cpu().numpy()
    got = np.concatenate([a, b], axis=1)
    assert first_mismatch(got, want) is None, first_mismatch(got, want)


def test_two_streams_per_xcd(torch_cuda, oracle):
    """B = 11: XCDs 0-2 carry two chain workgroups, the shared skip / conv1 workgroups serve both"""
    nl, B, T = 30, 11, 300
    d, blob, tensors, dil, mel, gc, seed_in, u, want = _mol_case(oracle, nl, B, T, frames=1)
    m = make_model(B, dil, tensors)
    assert m.fused_conditioning()
    got = m.generate(m.create_upsample(mel)[:, :T].contiguous(), gc, seed_in, u).cpu().numpy()
    assert first_mismatch(got, want) is None, first_mismatch(got, want)


@pytest.mark.parametrize("nl", [35, 40, 41, 50])
def test_second_chain_workgroup(torch_cuda, oracle, nl):
    """31-50 layers: wave 5 of the first chain workgroup hands on through L2, the second runs blocks of five from layer 30 (a block
    that ends at 35 and 40, one layer past 40, four full blocks); two calls"""
    B, T = 2, 600
    d, blob, tensors, dil, mel, gc, seed_in, u, want = _mol_case(oracle, nl, B, T, dil=_dil10(nl))
    m = make_model(B, dil, tensors)
    assert m.fused_conditioning()
    U = m.create_upsample(mel)
    a = m.generate(U[:, :400].contiguous(), gc, seed_in, u[:, :400]).cpu().numpy()
    b = m.generate(U[:, 400:600].contiguous(), gc, a[:, -1], u[:, 400:]).cpu().numpy()
    got = np.concatenate([a, b], axis=1)
    assert first_mismatch(got, want) is None, first_mismatch(got, want)


def test_teacher_forced_steps_through_both_chain_workgroups(torch_cuda, oracle):
    """priming at 41 layers: the end of a step comes back to the head from the second workgroup's third wave (one layer)"""
    _primed(torch_cuda, oracle, ([2 ** i for i in range(6)] * 9)[:41], 2, 200)


@pytest.mark.parametrize("nl", [11, 30])
def test_onehot_model(torch_cuda, oracle, nl):
    """the one-hot mu-law-256 model runs the same chain template with the same map: class ids equal to the checker's
    (pattern of tests/test_wavenet_gpu.py::test_xcd_onehot_kernel_shapes)"""
    B, T = 3, 300
    dil = _dil10(nl)
    d, tensors, blob = make_case(oracle, dil, scalar_input=False, S=512, Q=256, scale=0.12)
    m = make_model(B, dil, tensors, scalar_input=False, S=512, Q=256)
    assert m.fused_conditioning(), "the one-hot model must take the XCD kernel at S = 512, Q = 256"
    rng = np.random.RandomState(1)
    U = rng.uniform(-4, 4, (B, T, 80)).astype(np.float32)
    gc = (np.arange(B) % 2).astype(np.int32)
    seed_in = rng.randint(256, size=B).astype(np.int32)
    u, want = sensitive_onehot(oracle, d, blob, U, gc, seed_in, np.random.RandomState(2).random_sample((B, T)), 1.0)
    got = m.generate(U, gc, seed_in, u).cpu().numpy()
    assert got.dtype == np.int32
    assert np.array_equal(got, want), first_mismatch(got, want)
