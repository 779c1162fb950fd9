"""inputs under which SAMPLE EQUALITY against the oracle sees the network output (CPU only: the oracle is the one tool used).

Why: the generation tests compare drawn samples.  The MoL sampler clamps to +-1, and a clamped sample does not depend on the
network; the mixture logits act only through an argmax; a one-hot class id moves only when the draw sits next to a boundary of
the cumulative distribution.  With plain random weights and plain uniforms a kernel that is wrong by 0.1 % in one weight tensor
draws the same samples (tests/test_generation_inputs_cpu.py keeps that measurement as a test).  The uniforms are an injected
input of the C-ABI, so a test may choose them:

* shift_mol_head / narrow_logistic_uniforms take the MoL samples off the clamp, so that every sample is continuous in the mean
  and the log-scale of the selected component;
* knife_edge_mol puts the mixture SELECTION of every draw on its edge: the runner-up component's uniform is raised to the last
  float32 that keeps the winner (even step + stream) or the first that lets the runner-up win (odd);
* knife_edge_onehot puts every one-hot draw on the upper boundary of the class the plain draw selects: the last float64 that
  still gives the class (even step + stream) or the first that gives the next one (odd).

The builders step the oracle themselves (the sample of a step is the next step's input) and end by re-running
oracle.generate_mol / generate_mulaw on what they return: a builder cannot drift from the checker's own loop.

The conditions a test asserts ON THE ORACLE'S OUTPUT before it compares anything with the device are collected in
assert_mol_inputs / assert_onehot_inputs."""
import os
import pickle
import subprocess
import sys
import tempfile

import numpy as np

MOL_LO, MOL_HI = np.float32(1e-5), np.float32(1.0 - 1e-5)   # tf.random_uniform(minval=1e-5, maxval=1-1e-5), mixture.py:103,110
CLAMP_CAP = 0.05             # share of MoL samples that may sit on +-1 (the figure of tests/test_wavenet_wide_gpu.py)
EDGE_SHARE = 0.90            # share of the draws that must have received an edge
MIN_CLASSES, MIN_CLASSES_FROM = 50, 600        # one-hot: distinct classes wherever B * T >= 600
_U64_TOP = 1.0 - 2.0 ** -53  # the largest float64 below 1: np.random.random_sample never returns more


# ---------------------------------------------------------------------------------------------------------------- weights / uniforms
def shift_mol_head(tensors, out_channels, by=5.0):
    """a copy of `tensors` with the log-scale third of wavenet/conv1d_2/bias lowered by `by`: narrow mixture components, the
    samples leave the clamp.  Without that bias (use_bias=False) nothing can be shifted: the copy is returned as it is."""
    t = dict(tensors)
    if "wavenet/conv1d_2/bias" in t:
        b = np.array(t["wavenet/conv1d_2/bias"], np.float32, copy=True)
        b[2 * (out_channels // 3):] -= np.float32(by)
        t["wavenet/conv1d_2/bias"] = b
    return t


def narrow_logistic_uniforms(u):
    """a copy of MoL uniforms whose last column (the logistic draw, mixture.py:110) is mapped linearly from [1e-5, 1 - 1e-5] to
    0.5 +- 0.05: for models without biases, whose head cannot be shifted.  The selection columns are kept."""
    u = np.array(u, np.float32, copy=True)
    x = (u[..., -1].astype(np.float64) - float(MOL_LO)) / (float(MOL_HI) - float(MOL_LO))
    u[..., -1] = (0.45 + 0.1 * x).astype(np.float32)
    return u


# ---------------------------------------------------------------------------------------------------------------- conditions
def clamp_share(want):
    return float(np.mean(np.abs(np.asarray(want)) == 1.0))


def assert_off_the_clamp(want, cap=CLAMP_CAP):
    frac = clamp_share(want)
    assert frac <= cap, "the oracle's own samples sit on the clamp: %.1f %%" % (100 * frac)


def assert_edges(n_edges, n_draws, share=EDGE_SHARE):
    assert n_edges >= share * n_draws, "only %d of %d draws sit on an edge" % (n_edges, n_draws)


def assert_mol_inputs(u, want, n_edges, nr_mix=None):
    """the conditions of a MoL case: uniforms inside the range the C-ABI documents, at most 5 % of the oracle's samples on the
    clamp, an edge on at least 90 % of the draws (where there is more than one component to choose from)"""
    u = np.asarray(u)
    assert u.dtype == np.float32 and u.min() >= MOL_LO and u.max() <= MOL_HI, (u.dtype, u.min(), u.max())
    assert_off_the_clamp(want)
    if (u.shape[-1] - 1 if nr_mix is None else nr_mix) > 1:
        assert_edges(n_edges, np.asarray(want).size)


def assert_onehot_inputs(u, want, n_edges, Q):
    """the conditions of a one-hot case: float64 uniforms in [0, 1), an edge on at least 90 % of the draws, and at least 50
    distinct classes wherever there are 600 draws or more"""
    u = np.asarray(u); want = np.asarray(want)
    assert u.dtype == np.float64 and u.min() >= 0.0 and u.max() < 1.0, (u.dtype, u.min(), u.max())
    if Q > 1:
        assert_edges(n_edges, want.size)
    if want.size >= MIN_CLASSES_FROM and Q >= MIN_CLASSES:
        assert len(np.unique(want)) >= MIN_CLASSES, "only %d distinct classes in %d draws" % (len(np.unique(want)), want.size)


# ---------------------------------------------------------------------------------------------------------------- builders
def _edge(sample, s0, lo, top, est, widths):
    """sample(bits) -> outcome for the uniform with that bit pattern (the patterns of positive floats order like the floats);
    sample(lo) is s0.  Returns (a, a + 1, sample(a + 1)) with sample(a) == s0 != sample(a + 1), lo <= a < top, or None where
    sample(top) is still s0.  `est` is where the edge is expected: brackets of the given half-widths around it are tried first,
    then the whole range [lo, top] -- a bisection in every case, judged by the oracle's own sampler alone."""
    seen = {lo: s0}

    def keeps(bits):
        if bits not in seen:
            seen[bits] = sample(bits)
        return seen[bits] == s0

    a = b = None
    for w in widths if est is not None else ():
        ca, cb = max(lo, est - w), min(top, est + w)
        if ca < cb and keeps(ca) and not keeps(cb):
            a, b = ca, cb
            break
    if a is None:
        if lo >= top or keeps(top):
            return None
        a, b = lo, top
    while b - a > 1:                                                  # invariant: keeps(a), not keeps(b)
        mid = (a + b) // 2
        if keeps(mid):
            a = mid
        else:
            b = mid
    return a, b, seen[b]


_MOL_TOP = int(MOL_HI.view(np.int32))


def _mol_edge(O, y, u_row, nr, odd):
    """one draw: (uniforms with the edge placed, sample under them, True), or (u_row, sample, False) where no edge exists"""
    s0 = O.sample_mol(y, u_row)
    if nr < 2:
        return u_row, s0, False
    y64 = y[:nr].astype(np.float64)
    g = y64 - np.log(-np.log(u_row[:nr].astype(np.float64)))
    k = int(np.argmax(g))
    gk = g[k]
    g[k] = -np.inf
    r = int(np.argmax(g))                                             # the runner-up: the component whose uniform is raised
    trial = u_row.copy()
    cell = trial[r:r + 1].view(np.int32)

    def sample(bits):
        cell[0] = bits
        return O.sample_mol(y, trial)

    est = np.float32(np.exp(-np.exp(y64[r] - gk)))                    # where g_r meets g_k, in float64
    est = int(est.view(np.int32)) if MOL_LO < est < MOL_HI else None
    found = _edge(sample, s0, int(u_row[r:r + 1].view(np.int32)[0]), _MOL_TOP, est, (3, 64))
    if found is None:
        return u_row, s0, False                                       # the runner-up cannot win inside the uniform range
    a, b, sb = found
    cell[0] = b if odd else a
    return trial, (sb if odd else s0), True


def _primed_state(O, d, blob, gc, prime, n_streams):
    """a State after the teacher-forced steps of generate.py:168-180: prime (n_streams, n) inputs, zero local conditioning"""
    st = O.State(d, n_streams)
    if prime is not None:
        zeros = np.zeros((n_streams, d.L), np.float32) if d.L else None
        for i in range(prime.shape[1]):
            O.step(d, blob, st, prime[:, i], zeros, gc)
    return st


def _stream_job(O, b, d, blob, U, gc, first_input, u0, temperature, prime):
    """ONE stream (index b of the batch; the arrays hold this stream alone, leading axis 1): prime, then per step run the network,
    place the edge, draw, feed the sample back.  Returns (u, want, n_edges) of the stream."""
    st = _primed_state(O, d, blob, gc, prime, 1)
    T = u0.shape[1]
    u = u0.copy()
    want = np.empty((1, T), np.float32 if d.scalar_input else np.int32)
    inp = first_input.copy()
    n = 0
    for t in range(T):
        raw = O.step(d, blob, st, inp, None if U is None else U[:, t], gc)[0]
        if d.scalar_input:
            u[0, t], want[0, t], edge = _mol_edge(O, raw, u[0, t], u.shape[2] - 1, (t + b) & 1)
        else:
            u[0, t], want[0, t], edge = _onehot_edge(O, raw, temperature, float(u[0, t]), (t + b) & 1)
        n += edge
        inp = want[:, t].copy()
    return u, want, n


def _one(a, b):
    return None if a is None else np.ascontiguousarray(np.asarray(a)[b:b + 1])


def _in_worker_processes(O, workers, d, blob, per_stream, temperature):
    """the streams dealt out to `workers` fresh python processes that run this file (they only use the oracle); a list of
    (u, want, n_edges) in stream order"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(O.__file__)))
    with tempfile.TemporaryDirectory() as tmp:
        procs = []
        for w in range(workers):
            job = dict(dims=bytes(d), blob=blob, temperature=temperature, streams=per_stream[w::workers])
            with open(os.path.join(tmp, "job%d" % w), "wb") as f:
                pickle.dump(job, f, protocol=4)
            procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__), root, os.path.join(tmp, "job%d" % w),
                                           os.path.join(tmp, "out%d" % w)]))
        codes = [p.wait() for p in procs]
        assert not any(codes), "a builder process failed: %s" % codes
        parts = [None] * len(per_stream)
        for w in range(workers):
            with open(os.path.join(tmp, "out%d" % w), "rb") as f:
                parts[w::workers] = pickle.load(f)
    return parts


def _worker_main(root, job_path, out_path):
    sys.path.insert(0, root)
    from oracle import oracle as O
    with open(job_path, "rb") as f:
        job = pickle.load(f)
    d = O.Dims.from_buffer_copy(job["dims"])
    out = [_stream_job(O, b, d, job["blob"], U, gc, first, u0, job["temperature"], prime) for b, U, gc, first, u0, prime in job["streams"]]
    with open(out_path, "wb") as f:
        pickle.dump(out, f, protocol=4)


def _knife_edge(O, d, blob, U, gc, first_input, u0, temperature, prime, workers):
    B, T = u0.shape[:2]
    U = None if U is None else np.ascontiguousarray(U[:, :T], np.float32)
    prime = None if prime is None else np.ascontiguousarray(prime)
    per_stream = [(b, _one(U, b), _one(gc, b), _one(first_input, b), _one(u0, b), _one(prime, b)) for b in range(B)]
    workers = max(1, min(int(workers), B))
    if workers > 1:
        parts = _in_worker_processes(O, workers, d, blob, per_stream, temperature)
    else:                                            # one stream at a time: a stream's delay lines stay in the cache
        parts = [_stream_job(O, b, d, blob, U_, gc_, first_, u0_, temperature, prime_) for b, U_, gc_, first_, u0_, prime_ in per_stream]
    u = np.concatenate([p[0] for p in parts]); want = np.concatenate([p[1] for p in parts])
    n_edges = int(sum(p[2] for p in parts))
    # the closing run: the checker's own loop on the returned uniforms, all streams in one state, one stream per host thread
    st = _primed_state(O, d, blob, gc, prime, B)
    cores = O.set_threads(min(B, 16))
    try:
        if d.scalar_input:
            again = O.generate_mol(d, blob, st, U, gc, first_input, u)
        else:
            again = O.generate_mulaw(d, blob, st, U, gc, first_input, u, temperature)
    finally:
        O.set_threads(1)
    assert cores >= 1 and np.array_equal(again, want), "the builder's loop departs from the oracle's generate_* loop"
    return u, want, n_edges


def knife_edge_mol(O, d, blob, U, gc, first_input, u0, prime=None, workers=1):
    """U (B, T, L) upsampled rows or None, gc (B) ids / (B, G) embedding or None, first_input (B) float32, u0 (B, T, nr_mix + 1)
    plain uniforms.  Returns (u, want, n_edges): the uniforms with an edge on every draw that has one, the oracle's samples under
    them, and the number of draws that received an edge.  prime: (B, n) samples teacher-forced with zero local conditioning before
    the first step (generate.py:168-180).  workers: processes to deal the streams out to (long cases; same result)."""
    u0 = np.ascontiguousarray(u0, np.float32)
    assert u0.shape[2] - 1 == d.O // 3 and d.scalar_input
    return _knife_edge(O, d, blob, U, gc, np.ascontiguousarray(first_input, np.float32), u0, 1.0, prime, workers)


_U64_TOP_BITS = int(np.float64(_U64_TOP).view(np.int64))


def _onehot_edge(O, logits, temperature, u0, odd):
    """one draw: (u, class under u, True) with u on the upper boundary of the class u0 selects, or (u0, class, False)"""
    k, p = O.sample_categorical(logits, temperature, u0)

    def sample(bits):
        return O.sample_categorical(logits, temperature, float(np.int64(bits).view(np.float64)))[0]

    cdf = np.cumsum(p, dtype=np.float64)
    est = int(np.float64(min(cdf[k] / cdf[-1], _U64_TOP)).view(np.int64))  # the boundary in numpy's summation order: a few ulps off
    found = _edge(sample, k, int(np.float64(u0).view(np.int64)), _U64_TOP_BITS, est, (8, 256))
    if found is None:
        return u0, k, False                                           # the last non-empty class: no boundary below 1
    a, b, kb = found
    return (float(np.int64(b).view(np.float64)), kb, True) if odd else (float(np.int64(a).view(np.float64)), k, True)


def knife_edge_onehot(O, d, blob, U, gc, first_input, u0, temperature=1.0, prime=None, workers=1):
    """the one-hot counterpart: first_input (B) int32 class ids, u0 (B, T) float64 plain draws in [0, 1), prime (B, n) class ids.
    Returns (u, want, n_edges)."""
    u0 = np.ascontiguousarray(u0, np.float64)
    assert not d.scalar_input
    return _knife_edge(O, d, blob, U, gc, np.ascontiguousarray(first_input, np.int32), u0, float(temperature), prime, workers)


# ---------------------------------------------------------------------------------------------------------------- mutants
MUTANT_FACTOR = np.float32(1.0 + 2.0 ** -10)       # a 0.1 % error in one weight tensor


def mutants(d, tensors):
    """(label, exempt, tensors) for every tensor of the model scaled by float32(1 + 2^-10), one at a time; conv1d_2 of a MoL model
    is split into its logit / mean / log-scale columns.  exempt: the last layer's `dense` pair, whose output feeds nothing."""
    last = "wavenet/dilated_stack/layer%d/dilation_layer/dense/" % (d.n_layers - 1)
    for name in tensors:
        w = np.asarray(tensors[name], np.float32)
        if name.startswith("wavenet/conv1d_2/") and d.scalar_input:
            nr = d.O // 3
            parts = [("logits", 0, nr), ("means", nr, 2 * nr), ("log_scales", 2 * nr, 3 * nr)]
        else:
            parts = [(None, 0, w.shape[-1])]
        for tag, a, b in parts:
            m = w.copy()
            m[..., a:b] = m[..., a:b] * MUTANT_FACTOR
            t = dict(tensors); t[name] = m
            yield (name if tag is None else "%s[%s]" % (name, tag)), name.startswith(last), t


def changed_samples(got, want):
    """(number of differing samples, first differing step or None)"""
    bad = np.asarray(got) != np.asarray(want)
    return int(bad.sum()), (int(np.argmax(bad.any(axis=0))) if bad.any() else None)


if __name__ == "__main__":          # a builder process of _in_worker_processes
    _worker_main(*sys.argv[1:4])
