"""-m gpu: model.py:154's skip sum of the XCD generation kernel as a relay through the skip waves.

Wave v of skip workgroup g owns slice g of layers v, v + 8, ... of the served layers (all but the last, whose skip 1x1 runs in the
conv1 workgroups); LDS slot l of a stream holds the running total of layers 0 .. l, handed from the owner of layer l - 1 to the owner
of layer l, and the owner of the last served layer publishes.  The adds and their order are those of a single summing wave, so every
case compares with the CPU oracle bit for bit, under the inputs of tests/sensitive_inputs.py, T = 300 and short dilation lists."""
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


def _case(oracle, B, nl, use_bias=True, seed=0, steps=T, xcd_many=None):
    """(model, mel-conditioned inputs, the oracle's samples) of one MoL case on the XCD kernel"""
    dil = _dil(nl)
    d, tensors, blob = make_case(oracle, dil, use_bias=use_bias, shift=5.0)
    m = make_model(B, dil, tensors, use_bias=use_bias, xcd_many=xcd_many)
    assert m.kernel_name() == "wn_xcd_generate_kernel", m.kernel_name()
    rng = np.random.RandomState(100 * nl + B + seed)
    mel = rng.uniform(-4, 4, (B, 2, 80)).astype(np.float32)
    gc = (np.arange(B) % 2).astype(np.int32)
    first = (2 * rng.rand(B) - 1).astype(np.float32)
    U_o = oracle.upsample(d, blob, mel)[:, :steps]
    u, want = sensitive_mol(oracle, d, blob, U_o, gc, first, B, steps)
    return d, blob, m, mel, U_o, gc, first, u, want


def _run(m, mel, gc, first, u, steps=T):
    U = m.create_upsample(mel)[:, :steps].contiguous()
    return m.generate(U, gc, first, u).cpu().numpy()


@pytest.mark.parametrize("nl", [2, 3, 9, 10, 18])
def test_one_stream_per_xcd(torch_cuda, oracle, nl):
    """served layers 1 (no predecessor), 2 (one LDS hop), 8 (every wave once), 9 (the relay wraps round to wave 0's second layer),
    17 (two rounds and one more); sixteen conv1 workgroups behind them"""
    d, blob, m, mel, U_o, gc, first, u, want = _case(oracle, 8, nl)
    got = _run(m, mel, gc, first, u)
    assert np.array_equal(got, want), first_mismatch(got, want)


@pytest.mark.parametrize("B,xcd_many", [(9, None), (17, None), (25, 2)])
def test_two_to_four_streams_per_xcd(torch_cuda, oracle, B, xcd_many):
    """the blocking wait for the total below sits inside the stream loop; xcd_many = 2 keeps this kernel above batch 20"""
    d, blob, m, mel, U_o, gc, first, u, want = _case(oracle, B, 10, xcd_many=xcd_many)
    got = _run(m, mel, gc, first, u)
    assert np.array_equal(got, want), first_mismatch(got, want)


@pytest.mark.parametrize("B", [8, 9])
def test_one_layer_model_publishes_its_relu(torch_cuda, oracle, B):
    """no layer in front of the last one: the skip workgroups serve it themselves and publish relu(sum) of one term"""
    d, blob, m, mel, U_o, gc, first, u, want = _case(oracle, B, 1)
    got = _run(m, mel, gc, first, u)
    assert np.array_equal(got, want), first_mismatch(got, want)


@pytest.mark.parametrize("nl,B", [(31, 1), (42, 9), (50, 1)])
def test_31_to_50_layers(torch_cuda, oracle, nl, B):
    """the kernel for 31-50 layers: every tile in registers (31), one layer's tile per wave in LDS and two streams (42), wave 0
    with two LDS layers (50)"""
    d, blob, m, mel, U_o, gc, first, u, want = _case(oracle, B, nl, steps=200)
    got = _run(m, mel, gc, first, u, steps=200)
    assert np.array_equal(got, want), first_mismatch(got, want)


def test_onehot_model(torch_cuda, oracle):
    nl, B = 10, 8
    dil = _dil(nl)
    d, tensors, blob = make_case(oracle, dil, scalar_input=False, S=512, Q=256, scale=0.12)
    m = make_model(B, dil, tensors, scalar_input=False, S=512, Q=256)
    assert m.kernel_name() == "wn_xcd_generate_kernel", m.kernel_name()
    rng = np.random.RandomState(1)
    U = rng.uniform(-4, 4, (B, T, 80)).astype(np.float32)
    gc = (np.arange(B) % 2).astype(np.int32)
    seed_in = rng.randint(256, size=B).astype(np.int32)
    u, want = sensitive_onehot(oracle, d, blob, U, gc, seed_in, np.random.RandomState(2).random_sample((B, T)), 1.0)
    got = m.generate(U, gc, seed_in, u).cpu().numpy()
    assert np.array_equal(got, want), first_mismatch(got, want)


def test_no_biases(torch_cuda, oracle):
    d, blob, m, mel, U_o, gc, first, u, want = _case(oracle, 8, 10, use_bias=False)
    got = _run(m, mel, gc, first, u)
    assert np.array_equal(got, want), first_mismatch(got, want)


def test_three_calls_of_unequal_length_equal_one(torch_cuda, oracle):
    """tags and the LDS slots across launches: one utterance in calls of 1, 100 and 199 steps"""
    d, blob, m, mel, U_o, gc, first, u, want = _case(oracle, 9, 10, seed=1)
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


def test_raw_conv1d_2_outputs_of_the_layer_dumps(torch_cuda, oracle):
    """a wrong total that the sampler's clamp or argmax would hide: the raw network outputs of the first 20 steps"""
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
