"""-m gpu: the waits on the XCD generation kernel's sample-to-sample path as bare spins with the watchdog's loop behind them.

Every wait of the path (the chain's hand-offs through LDS and, above 30 layers, through L2; the skip workgroups' last served layer;
the conv1 workgroups' sum granule and arrival counters; the one-hot model's h2 gather; the teacher-forced head's end-of-step wait)
takes `spin_looks` looks at its word with nothing but the load and the compare in the loop, then falls into the poll_tick loop it
used to be.  The option "spin_looks" = 1 sends every wait of every step through that hand-over while the kernel runs normally.
Every case compares with the CPU oracle bit for bit, under the inputs of tests/sensitive_inputs.py, T = 300 (200 where noted) and
short dilation lists; no case makes a wait time out."""
import functools

import numpy as np
import pytest

from helpers import first_mismatch, make_case, make_model, sensitive_mol, sensitive_onehot

pytestmark = pytest.mark.gpu

T = 300


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def _dil(nl):
    return ([1, 2, 4, 8, 16, 32, 64] * 8)[:nl]


@functools.lru_cache(maxsize=None)
def _mol_reference(oracle, B, nl, steps, seed):
    """(dims, tensors, blob, inputs, the oracle's samples) of one MoL case: computed once and shared (nobody writes to it)"""
    dil = _dil(nl)
    d, tensors, blob = make_case(oracle, dil, shift=5.0)
    rng = np.random.RandomState(100 * nl + B + seed)
    mel = rng.uniform(-4, 4, (B, 2, 80)).astype(np.float32)
    gc = (np.arange(B) % 2).astype(np.int32)
    first = (2 * rng.rand(B) - 1).astype(np.float32)
    U_o = oracle.upsample(d, blob, mel)[:, :steps]
    u, want = sensitive_mol(oracle, d, blob, U_o, gc, first, B, steps)
    return d, tensors, blob, mel, U_o, gc, first, u, want


def _case(oracle, B, nl, steps=T, seed=0, spin_looks=None):
    d, tensors, blob, mel, U_o, gc, first, u, want = _mol_reference(oracle, B, nl, steps, seed)
    m = make_model(B, _dil(nl), tensors)
    assert m.kernel_name() == "wn_xcd_generate_kernel", m.kernel_name()
    if spin_looks is not None:
        m.set_option("spin_looks", spin_looks)
    return d, blob, m, mel, U_o, gc, first, u, want


def _run(m, mel, gc, first, u, steps=T):
    U = m.create_upsample(mel)[:, :steps].contiguous()
    return m.generate(U, gc, first, u).cpu().numpy()


@functools.lru_cache(maxsize=None)
def _onehot_reference(oracle):
    nl, B = 10, 8
    d, tensors, blob = make_case(oracle, _dil(nl), scalar_input=False, S=512, Q=256, scale=0.12)
    rng = np.random.RandomState(1)
    U = rng.uniform(-4, 4, (B, T, 80)).astype(np.float32)
    gc = (np.arange(B) % 2).astype(np.int32)
    seed_in = rng.randint(256, size=B).astype(np.int32)
    u, want = sensitive_onehot(oracle, d, blob, U, gc, seed_in, np.random.RandomState(2).random_sample((B, T)), 1.0)
    return tensors, U, gc, seed_in, u, want


def _onehot(oracle, spin_looks=None):
    tensors, U, gc, seed_in, u, want = _onehot_reference(oracle)
    m = make_model(8, _dil(10), tensors, scalar_input=False, S=512, Q=256)
    assert m.kernel_name() == "wn_xcd_generate_kernel", m.kernel_name()
    if spin_looks is not None:
        m.set_option("spin_looks", spin_looks)
    got = m.generate(U, gc, seed_in, u).cpu().numpy()
    assert np.array_equal(got, want), first_mismatch(got, want)


@pytest.mark.parametrize("nl,steps", [(1, T), (5, T), (6, T), (11, T), (30, 200)])
def test_one_stream_per_xcd(torch_cuda, oracle, nl, steps):
    """chain waves: none in front of the last layer's fold (1); ONE full last wave with immediate stores (5); a deferring wave and a
    wave of one layer with the count at run time (6); three waves (11); all six (30, 200 steps)"""
    d, blob, m, mel, U_o, gc, first, u, want = _case(oracle, 8, nl, steps=steps)
    got = _run(m, mel, gc, first, u, steps=steps)
    assert np.array_equal(got, want), first_mismatch(got, want)


@pytest.mark.parametrize("B", [9, 17])
def test_several_streams_per_xcd(torch_cuda, oracle, B):
    """eight conv1 workgroups; the waits sit inside the loop over the XCD's streams"""
    d, blob, m, mel, U_o, gc, first, u, want = _case(oracle, B, 10)
    got = _run(m, mel, gc, first, u)
    assert np.array_equal(got, want), first_mismatch(got, want)


def test_onehot_model(torch_cuda, oracle):
    """the one-hot conv1 workgroups (two arrival counters, the h2 gather) and the head's logits poll"""
    _onehot(oracle)


@pytest.mark.parametrize("nl,B", [(31, 1), (42, 9)])
def test_second_chain_workgroup(torch_cuda, oracle, nl, B):
    """the hand-off to the second chain workgroup is an L2 granule: the L2 form of the spin (200 steps)"""
    d, blob, m, mel, U_o, gc, first, u, want = _case(oracle, B, nl, steps=200)
    got = _run(m, mel, gc, first, u, steps=200)
    assert np.array_equal(got, want), first_mismatch(got, want)


@pytest.mark.parametrize("nl,spin_looks", [(6, None), (6, 1), (31, None)])
def test_teacher_forced_priming_then_sampling(torch_cuda, oracle, nl, spin_looks):
    """twv_wavenet_prime: the head waits for the end of the step in LDS box 8 (6 layers) or the DONE granule (31), with the tag of the
    step before"""
    dil = ([1, 2, 4, 8, 16, 32] * 6)[:nl]
    B, steps = 3, 200
    d, tensors, blob = make_case(oracle, dil, shift=5.0)
    m = make_model(B, dil, tensors)
    assert m.kernel_name() == "wn_xcd_generate_kernel", m.kernel_name()
    if spin_looks is not None:
        m.set_option("spin_looks", spin_looks)
    rf = oracle.receptive_field(d)
    rng = np.random.RandomState(9 + nl)
    seedwave = rng.uniform(-1, 1, (B, rf)).astype(np.float32)
    mel = rng.uniform(-4, 4, (B, 1, 80)).astype(np.float32)
    gc = (np.arange(B) % 2).astype(np.int32)
    U_o = oracle.upsample(d, blob, mel)[:, :steps]
    u, want = sensitive_mol(oracle, d, blob, U_o, gc, seedwave[:, -1], B, steps, prime=seedwave[:, :rf - 1])
    m.prime(seedwave[:, :rf - 1], None, gc)
    got = m.generate(m.create_upsample(mel)[:, :steps].contiguous(), gc, seedwave[:, -1], u).cpu().numpy()
    assert np.array_equal(got, want), first_mismatch(got, want)


def test_three_launches_equal_one(torch_cuda, oracle):
    """tags start again in every launch: one utterance in launches of 1, 100 and 199 steps"""
    d, blob, m, mel, U_o, gc, first, u, want = _case(oracle, 8, 10)
    U = m.create_upsample(mel)[:, :T].contiguous()
    outs, fi, p = [], first, 0
    for n in (1, 100, 199):
        o = m.generate(U[:, p:p + n].contiguous(), gc, fi, u[:, p:p + n]).cpu().numpy()
        outs.append(o)
        fi, p = o[:, -1], p + n
    got = np.concatenate(outs, axis=1)
    assert np.array_equal(got, want), first_mismatch(got, want)
    m.queue_initializer()
    once = m.generate(U, gc, first, u).cpu().numpy()
    assert np.array_equal(once, want), first_mismatch(once, want)


@pytest.mark.parametrize("spin_looks", [1, 2])
def test_fallback_on_every_wait_mol(torch_cuda, oracle, spin_looks):
    """one (two) bare looks, then the watchdog's loop, on every wait of every step: the same bits"""
    d, blob, m, mel, U_o, gc, first, u, want = _case(oracle, 8, 10, spin_looks=spin_looks)
    got = _run(m, mel, gc, first, u)
    assert np.array_equal(got, want), first_mismatch(got, want)


@pytest.mark.parametrize("spin_looks", [1, 2])
def test_fallback_on_every_wait_onehot(torch_cuda, oracle, spin_looks):
    _onehot(oracle, spin_looks=spin_looks)


@pytest.mark.parametrize("spin_looks", [1, 2])
def test_fallback_on_every_wait_second_chain_workgroup(torch_cuda, oracle, spin_looks):
    d, blob, m, mel, U_o, gc, first, u, want = _case(oracle, 1, 31, steps=200, spin_looks=spin_looks)
    got = _run(m, mel, gc, first, u, steps=200)
    assert np.array_equal(got, want), first_mismatch(got, want)


@pytest.mark.parametrize("value", [0, 70000])
def test_option_range(torch_cuda, oracle, value):
    import twvk_amd
    d, tensors, blob = _mol_reference(oracle, 8, 10, T, 0)[:3]
    m = make_model(8, _dil(10), tensors)
    with pytest.raises(twvk_amd._lib.TwvError, match="spin_looks"):
        m.set_option("spin_looks", value)
    m.set_option("spin_looks", 65535)
    m.set_option("spin_looks", 1)


def test_raw_conv1d_2_outputs_of_the_layer_dumps(torch_cuda, oracle):
    """the instrumented build takes the same waits: the raw network outputs of the first 20 steps (what the sampler's clamp or argmax
    would hide)"""
    nl, B, dbg = 10, 2, 20
    d, blob, m, mel, U_o, gc, first, u, want = _case(oracle, B, nl)
    U = m.create_upsample(mel)[:, :T].contiguous()
    got, dump = m.generate(U, gc, first, u, debug_steps=dbg)
    got, dump = got.cpu().numpy(), dump.cpu().numpy()
    st = oracle.State(d, B)
    inp = first.copy()
    for t in range(dbg):
        raw, dz, dx = oracle.step(d, blob, st, inp, U_o[:, t], gc, debug=True)
        graw = dump[:, t, nl * 64:nl * 64 + d.O]
        assert np.array_equal(graw, raw), ("raw", t, first_mismatch(graw, raw))
        inp = want[:, t]
    assert np.array_equal(got, want), first_mismatch(got, want)
