"""The inputs of the generation tests discriminate (CPU only, the oracle against itself).

Sample equality against the oracle is only as strong as the inputs in front of it.  For every configuration of
tests/sensitive_inputs.py that the GPU tests use, this file builds the inputs on a small stack, then scales ONE weight tensor by
float32(1 + 2^-10) -- a kernel wrong by 0.1 % in that tensor -- runs the oracle on the SAME inputs and asserts that at least one
sample moves.  Every tensor of the model is tried, one at a time (conv1d_2 of a MoL model as its logit / mean / log-scale
columns); the one survivor allowed is the last layer's `dense` pair, whose output feeds nothing.

The second half keeps the measurement that made the builders necessary, on the inputs the suite used before: under plain
random_sample uniforms no 0.1 % mutant of the one-hot model changes a single class id, under plain mol_uniforms the mixture-logit
mutant changes nothing and more than half of the oracle's samples are +-1.  If someone "simplifies" the GPU tests back to those
inputs, this is the file that says what is lost.  scripts/generation_input_sensitivity.py prints the whole table."""
import numpy as np
import pytest

import sensitive_inputs as SI
from helpers import mol_uniforms

DIL = [1, 2, 4, 8, 16, 1, 2]
B, T, S = 3, 70, 128

#            name                     model     kwargs
CONFIGS = [("mol_shifted_0.05", dict(scalar=True, scale=0.05)),
           ("mol_shifted_0.10", dict(scalar=True, scale=0.1)),
           ("mol_no_bias_narrowed", dict(scalar=True, scale=0.05, use_bias=False)),
           ("mol_wide_64x64", dict(scalar=True, scale=0.05, R=64, D=64)),
           ("onehot_0.05", dict(scalar=False, scale=0.05)),
           ("onehot_0.12", dict(scalar=False, scale=0.12)),
           ("onehot_0.30_t0.8", dict(scalar=False, scale=0.3, temperature=0.8)),
           ("onehot_wide_64x64_0.30", dict(scalar=False, scale=0.3, R=64, D=64))]


class Case:
    """one model + inputs; rerun(tensors) gives the oracle's samples for other weights on the same inputs"""

    def __init__(self, O, scalar, scale, use_bias=True, R=32, D=32, temperature=1.0, dil=DIL, B=B, T=T, S=S, knife_edge=True,
                 shift=True, u_seed=2, direct_lc=False):
        self.O, self.scalar, self.temperature, self.B, self.T = O, scalar, temperature, B, T
        self.d = d = O.make_dims(dil, R=R, D=D, S=S, scalar_input=scalar, use_bias=use_bias)
        t = O.random_tensors(d, seed=0, scale=scale)
        self.tensors = SI.shift_mol_head(t, d.O) if (scalar and shift) else dict(t)
        rng = np.random.RandomState(1)
        # direct_lc: the upsampled rows drawn directly, as _run_onehot of tests/test_wavenet_gpu.py does (no upsampling network)
        self.mel = rng.uniform(-4, 4, (B, T, 80) if direct_lc else (B, 1, 80)).astype(np.float32)
        self.direct_lc = direct_lc
        self.gc = (np.arange(B) % 2).astype(np.int32)
        if scalar:
            self.first = (2 * rng.rand(B) - 1).astype(np.float32)
            u0 = mol_uniforms(B, T, d.O // 3, seed=u_seed)
            if not use_bias and shift:
                u0 = SI.narrow_logistic_uniforms(u0)
        else:
            self.first = rng.randint(d.Q, size=B).astype(np.int32)
            u0 = np.random.RandomState(u_seed).random_sample((B, T))
        blob = O.blob_from_tensors(d, self.tensors)
        U = self.mel if direct_lc else O.upsample(d, blob, self.mel)[:, :T].copy()
        if not knife_edge:
            self.u, self.n_edges = u0, 0
            self.want = self.rerun(self.tensors)
        elif scalar:
            self.u, self.want, self.n_edges = SI.knife_edge_mol(O, d, blob, U, self.gc, self.first, u0)
        else:
            self.u, self.want, self.n_edges = SI.knife_edge_onehot(O, d, blob, U, self.gc, self.first, u0, temperature)

    def rerun(self, tensors):
        O, d = self.O, self.d
        blob = O.blob_from_tensors(d, tensors)
        U = self.mel if self.direct_lc else O.upsample(d, blob, self.mel)[:, :self.T].copy()   # the upsampling kernels are weights too
        if self.scalar:
            return O.generate_mol(d, blob, O.State(d, self.B), U, self.gc, self.first, self.u)
        return O.generate_mulaw(d, blob, O.State(d, self.B), U, self.gc, self.first, self.u, self.temperature)

    def table(self):
        """[(label, exempt, changed samples, first differing step)] over every mutant"""
        return [(label, exempt) + SI.changed_samples(self.rerun(t), self.want) for label, exempt, t in SI.mutants(self.d, self.tensors)]


@pytest.mark.parametrize("name,kw", CONFIGS, ids=[c[0] for c in CONFIGS])
def test_every_mutant_is_killed(oracle, name, kw):
    c = Case(oracle, **kw)
    if c.scalar:
        SI.assert_mol_inputs(c.u, c.want, c.n_edges)
    else:
        SI.assert_onehot_inputs(c.u, c.want, c.n_edges, c.d.Q)
    rows = c.table()
    classes = {label.split("/")[-2] + "/" + label.split("/")[-1] for label, _, _, _ in rows}
    want_classes = {"conv1d/kernel", "gc_embedding", "conv_filter/kernel", "conv_gate/kernel", "gc_filter/kernel", "gc_gate/kernel",
                    "lc_filter/kernel", "lc_gate/kernel", "dense/kernel", "skip/kernel", "conv1d_1/kernel", "upsample0/kernel"}
    assert want_classes <= {k.replace("wavenet/", "") for k in classes}, sorted(classes)
    survivors = [label for label, exempt, n, _ in rows if n == 0]
    exempt = [label for label, ex, _, _ in rows if ex]
    assert len(exempt) == (2 if kw.get("use_bias", True) else 1)
    assert survivors == exempt, "mutants that change no sample: %s" % survivors      # the last layer's dense pair and nothing else
    killed = sorted(n for _, ex, n, _ in rows if not ex)
    assert killed[len(killed) // 2] >= (B * T) // 4, killed                               # measured: the median mutant moves 100-210 of 210


def test_builders_do_not_depend_on_the_worker_count_and_prime_like_the_checker(oracle):
    """streams dealt out to worker processes give the same inputs; `prime` is the teacher-forced run of generate.py:168-180"""
    c = Case(oracle, scalar=True, scale=0.05, T=20)
    blob = oracle.blob_from_tensors(c.d, c.tensors)
    U = oracle.upsample(c.d, blob, c.mel)[:, :c.T].copy()
    prime = np.random.RandomState(4).uniform(-1, 1, (B, 40)).astype(np.float32)
    one = SI.knife_edge_mol(oracle, c.d, blob, U, c.gc, c.first, mol_uniforms(B, c.T, 10), prime=prime)
    two = SI.knife_edge_mol(oracle, c.d, blob, U, c.gc, c.first, mol_uniforms(B, c.T, 10), prime=prime, workers=2)
    assert np.array_equal(one[0], two[0]) and np.array_equal(one[1], two[1]) and one[2] == two[2]
    st = oracle.State(c.d, B)
    for i in range(40):
        oracle.step(c.d, blob, st, prime[:, i], np.zeros((B, 80), np.float32), c.gc)
    assert np.array_equal(oracle.generate_mol(c.d, blob, st, U, c.gc, c.first, one[0]), one[1])
    assert not np.array_equal(one[1], c.want)                                            # the primed state matters


def test_edges_are_adjacent_values(oracle):
    """what an edge is: the neighbouring uniform on the other side of it gives another sample"""
    c = Case(oracle, scalar=False, scale=0.05, T=12)
    blob = oracle.blob_from_tensors(c.d, c.tensors)
    U = oracle.upsample(c.d, blob, c.mel)[:, :c.T].copy()
    st = oracle.State(c.d, B)
    inp = c.first
    for t in range(c.T):
        raw = oracle.step(c.d, blob, st, inp, U[:, t], c.gc)
        for b in range(B):
            u = c.u[b, t]
            other = np.nextafter(u, 0.0 if (t + b) & 1 else 1.0)
            k, _ = oracle.sample_categorical(raw[b], 1.0, u)
            k2, _ = oracle.sample_categorical(raw[b], 1.0, other)
            assert k == c.want[b, t] and k2 != k and abs(k2 - k) >= 1, (b, t, k, k2)
        inp = c.want[:, t]
    m = Case(oracle, scalar=True, scale=0.05, T=12)
    blob = oracle.blob_from_tensors(m.d, m.tensors)
    U = oracle.upsample(m.d, blob, m.mel)[:, :m.T].copy()
    u0 = mol_uniforms(B, m.T, 10)
    st = oracle.State(m.d, B)
    inp = m.first
    for t in range(m.T):
        raw = oracle.step(m.d, blob, st, inp, U[:, t], m.gc)
        for b in range(B):
            col = np.flatnonzero(m.u[b, t] != u0[b, t])
            assert col.size == 1 and col[0] < 10 and m.u[b, t, col[0]] > u0[b, t, col[0]]      # one selection uniform, raised
            other = m.u[b, t].copy()
            other[col[0]] = (other[col[0]:col[0] + 1].view(np.int32) + (-1 if (t + b) & 1 else 1)).view(np.float32)[0]
            assert oracle.sample_mol(raw[b], m.u[b, t]) == m.want[b, t] != oracle.sample_mol(raw[b], other), (b, t)
        inp = m.want[:, t]


def test_shift_and_narrowing_helpers(oracle):
    d = oracle.make_dims(DIL, S=S)
    t = oracle.random_tensors(d, seed=0)
    s = SI.shift_mol_head(t, 30)
    assert s is not t and np.array_equal(s["wavenet/conv1d_2/bias"][:20], t["wavenet/conv1d_2/bias"][:20])
    assert np.array_equal(s["wavenet/conv1d_2/bias"][20:], t["wavenet/conv1d_2/bias"][20:] - np.float32(5))
    assert all(s[k] is t[k] for k in t if k != "wavenet/conv1d_2/bias")
    nb = oracle.random_tensors(oracle.make_dims(DIL, S=S, use_bias=False), seed=0)
    assert SI.shift_mol_head(nb, 30).keys() == nb.keys()                                   # nothing to shift: a no-op
    u = mol_uniforms(4, 500, 10)
    n = SI.narrow_logistic_uniforms(u)
    assert np.array_equal(n[..., :10], u[..., :10]) and n.dtype == np.float32
    assert n[..., 10].min() >= 0.45 and n[..., 10].max() <= 0.55 and n[..., 10].std() > 0.02
    with pytest.raises(AssertionError, match="clamp"):
        SI.assert_off_the_clamp(np.array([1.0, -1.0, 0.3, 0.2], np.float32))
    with pytest.raises(AssertionError, match="edge"):
        SI.assert_edges(80, 100)


# ---------------------------------------------------------------------------------------------------------------- the contrast
NINE = ["wavenet/conv1d/kernel", "wavenet/gc_embedding", "wavenet/dilated_stack/layer0/dilation_layer/conv_filter/kernel",
        "wavenet/dilated_stack/layer2/dilation_layer/conv_gate/kernel", "wavenet/dilated_stack/layer1/dilation_layer/lc_filter/kernel",
        "wavenet/dilated_stack/layer0/dilation_layer/dense/kernel", "wavenet/dilated_stack/layer3/dilation_layer/skip/kernel",
        "wavenet/conv1d_1/kernel", "wavenet/conv1d_2/kernel"]


@pytest.mark.parametrize("scale", [0.05, 0.12, 0.3])
def test_contrast_plain_uniforms_hide_every_onehot_mutant(oracle, scale):
    """the inputs of _run_onehot / _onehot_xcd_case / the dump tests before this file existed: [1, 2, 4, 8, 16], B = 3, T = 50,
    plain random_sample draws.  A 0.1 % error in any of nine tensors changes 0 of 150 class ids -- and the same nine mutants are
    killed by the knife-edge draws"""
    kw = dict(scalar=False, scale=scale, dil=[1, 2, 4, 8, 16], T=50, direct_lc=True)
    plain, edged = Case(oracle, knife_edge=False, **kw), Case(oracle, **kw)
    for c, killed in ((plain, False), (edged, True)):
        rows = {label: n for label, _, n, _ in c.table()}
        for name in NINE:
            assert (rows[name] > 0) == killed, (name, rows[name], "knife-edge" if killed else "plain")


def test_contrast_plain_mol_inputs_sit_on_the_clamp_and_hide_the_logits(oracle):
    """the inputs of test_generate_variants before: 7 layers, scale 0.1, S = 512, unshifted, plain mol_uniforms"""
    kw = dict(scalar=True, scale=0.1, S=512)
    plain = Case(oracle, knife_edge=False, shift=False, **kw)
    assert SI.clamp_share(plain.want) > 0.5, SI.clamp_share(plain.want)
    rows = {label: n for label, _, n, _ in plain.table()}
    assert rows["wavenet/conv1d_2/kernel[logits]"] == 0 and rows["wavenet/conv1d_2/bias[logits]"] == 0
    shifted_only = Case(oracle, knife_edge=False, scalar=True, scale=0.05)             # off the clamp, plain selection uniforms
    assert SI.clamp_share(shifted_only.want) == 0.0
    rows = {label: n for label, _, n, _ in shifted_only.table()}
    assert rows["wavenet/conv1d_2/kernel[logits]"] == 0                                 # the logits stay invisible without the edges
    assert rows["wavenet/conv1d_2/kernel[means]"] > (B * T) // 2
