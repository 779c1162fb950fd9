"""-m gpu: the conv1 stage of the XCD generation kernel in half-chunk form.

The summing waves of a conv1 workgroup run their conv1d_2 chunk as a dense half chunk (16 DPP fmacs per lane, operand in the Z
layout, outputs in the order of dpp_dense_out), and at one stream per XCD (batch <= 8, MoL, 2..30 layers) the stage runs on
sixteen workgroups, one per (output block, output half).  Every case compares with the CPU oracle bit for bit under the inputs
of tests/sensitive_inputs.py (shifted head, every mixture selection on its edge), T = 450 and short dilation lists."""
import numpy as np
import pytest

from helpers import first_mismatch, make_case, make_model, sensitive_mol

pytestmark = pytest.mark.gpu

T = 450


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def _dil(nl):
    return ([1, 2, 4, 8, 16, 32, 64] * 5)[:nl]


def _case(oracle, B, nl, out_channels=30, use_bias=True, seed=0, prime=False, steps=T):
    """(model, mel-conditioned inputs, the oracle's samples) of one MoL case on the XCD kernel; prime: receptive field - 1
    teacher-forced samples in front (generate.py:168-180)"""
    dil = _dil(nl)
    d, tensors, blob = make_case(oracle, dil, out_channels=out_channels, use_bias=use_bias, shift=5.0)
    m = make_model(B, dil, tensors, out_channels=out_channels, use_bias=use_bias)
    assert m.kernel_name() == "wn_xcd_generate_kernel", m.kernel_name()
    rng = np.random.RandomState(100 * nl + B + seed)
    mel = rng.uniform(-4, 4, (B, 2, 80)).astype(np.float32)
    gc = (np.arange(B) % 2).astype(np.int32)
    if prime:
        seedwave = rng.uniform(-1, 1, (B, oracle.receptive_field(d))).astype(np.float32)
        first = seedwave[:, -1]
    else:
        seedwave = None
        first = (2 * rng.rand(B) - 1).astype(np.float32)
    U_o = oracle.upsample(d, blob, mel)[:, :steps]
    u, want = sensitive_mol(oracle, d, blob, U_o, gc, first, B, steps, prime=seedwave[:, :-1] if prime else None)
    return d, blob, m, mel, U_o, gc, first, seedwave, u, want


@pytest.mark.parametrize("nl", [2, 6, 30])
@pytest.mark.parametrize("B", [1, 3, 8])
def test_one_stream_per_xcd(torch_cuda, oracle, B, nl):
    """NL = 2: the smallest model whose last skip 1x1 runs in the conv1 workgroups; NL = 6: one layer into the second chain wave;
    B = 1, 3 leave XCDs idle"""
    d, blob, m, mel, U_o, gc, first, _, u, want = _case(oracle, B, nl)
    got = m.generate(m.create_upsample(mel), gc, first, u).cpu().numpy()
    assert np.array_equal(got, want), first_mismatch(got, want)


@pytest.mark.parametrize("use_bias", [True, False])
@pytest.mark.parametrize("out_channels", [30, 3])
def test_padding_outputs_and_bias_lanes(torch_cuda, oracle, out_channels, use_bias):
    """outputs >= O of the conv1d_2 half tile are padding (their slots are still written: the sampler checks every tag); the bias
    lanes of conv1d_1 and of the last layer's skip 1x1 follow the permuted lane map"""
    d, blob, m, mel, U_o, gc, first, _, u, want = _case(oracle, 8, 6, out_channels=out_channels, use_bias=use_bias)
    got = m.generate(m.create_upsample(mel), gc, first, u).cpu().numpy()
    assert np.array_equal(got, want), first_mismatch(got, want)


def test_three_calls_of_unequal_length_equal_one(torch_cuda, oracle):
    """tags, the LDS arrival counter and the state across launches: one utterance in calls of 1, 160 and 289 steps"""
    d, blob, m, mel, U_o, gc, first, _, u, want = _case(oracle, 8, 6, seed=1)
    U = m.create_upsample(mel)[:, :T].contiguous()
    outs, fi, p = [], first, 0
    for n in (1, 160, T - 161):
        o = m.generate(U[:, p:p + n].contiguous(), gc, fi, u[:, p:p + n]).cpu().numpy()
        outs.append(o)
        fi, p = o[:, -1], p + n
    got = np.concatenate(outs, axis=1)
    assert np.array_equal(got, want), first_mismatch(got, want)
    m.queue_initializer()
    once = m.generate(U, gc, first, u).cpu().numpy()
    assert np.array_equal(once, want), first_mismatch(once, want)


def test_prime_then_generate(torch_cuda, oracle):
    """the conv1 workgroups idle through the teacher-forced launch and must still take their tickets"""
    d, blob, m, mel, U_o, gc, first, seedwave, u, want = _case(oracle, 3, 6, prime=True)
    m.prime(seedwave[:, :-1], None, gc)
    got = m.generate(m.create_upsample(mel), gc, first, u).cpu().numpy()
    assert np.array_equal(got, want), first_mismatch(got, want)


@pytest.mark.parametrize("B,nl", [(9, 6), (8, 1)])
def test_eight_workgroup_role_where_the_split_does_not_apply(torch_cuda, oracle, B, nl):
    """two streams on an XCD (B = 9) and a model without a layer in front of the folded one (NL = 1) keep eight conv1 workgroups:
    the role-table arithmetic of host and device (a disagreement ends in status 90 or a watchdog code, not in samples)"""
    d, blob, m, mel, U_o, gc, first, _, u, want = _case(oracle, B, nl)
    got = m.generate(m.create_upsample(mel), gc, first, u).cpu().numpy()
    assert np.array_equal(got, want), first_mismatch(got, want)


def test_raw_conv1d_2_outputs_of_the_layer_dumps(torch_cuda, oracle):
    """a wrong chunk partial that the sampler's clamp or argmax would hide: the raw network outputs of the first 20 steps"""
    nl, B, dbg = 6, 2, 20
    d, blob, m, mel, U_o, gc, first, _, u, want = _case(oracle, B, nl)
    got, dump = m.generate(m.create_upsample(mel), gc, first, u, debug_steps=dbg)
    got, dump = got.cpu().numpy(), dump.cpu().numpy()
    st = oracle.State(d, B)
    inp = first.copy()
    for t in range(dbg):
        raw, dz, dx = oracle.step(d, blob, st, inp, U_o[:, t], gc, debug=True)
        graw = dump[:, t, nl * 64:nl * 64 + d.O]
        assert np.array_equal(graw, raw), ("raw", t, first_mismatch(graw, raw))
        inp = want[:, t]
    assert np.array_equal(got, want), first_mismatch(got, want)
