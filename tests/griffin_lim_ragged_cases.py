"""The cases of the ragged Griffin-Lim tests (tests/test_griffin_lim_ragged_cpu.py, tests/test_griffin_lim_ragged_gpu.py) and of the
ragged rows of scripts/griffin_lim_parity.py -- TEST INFRASTRUCTURE ONLY, host code.

Utterances of unequal lengths run in ONE call; every utterance is held to the bar of tests/griffin_lim_cases.py against the float64
checker run on that utterance ALONE, at its own length: e_gpu <= max(8 x e_f32, 1e-6), never above G.OLD_BAR.  Utterance i of a case
is G.inputs(n_fft, T_i, 1, seed)[.][0] with a seed per (case, iters, i).  Checker runs are cached: computed once, shared, read-only."""
import numpy as np

import audio_analysis_ref as R
import griffin_lim_cases as G

# name -> (n_fft, win, hop), frames per utterance, iterations, pre-emphasis k's, distinct utterances (None: all), what it pins
CASES = {
    "A": ((128, 128, 32), [20, 4, 11], (0, 3), (0.97,), None),                 # the shortest accepted (4) between two others
    "B": ((128, 101, 25), [21, 4, 9, 21, 5], (0, 3), (0.97,), None),           # odd window, equal lengths apart, a short last one
    "C": ((64, 32, 40), [12, 2, 3], (0, 3), (0.97,), None),                    # hop > win, T = 2 inside a batch
    "D": ((64, 64, 11), [4, 9, 4], (0, 3), (0.97,), None),                     # len = n_fft/2 + 1 first and last
    "E": ((64, 48, 40), [2, 2, 7], (0, 3), (0.97,), None),                     # two T = 2 neighbours
    "F": ((2048, 1200, 300), [14, 5, 9], (0, 3), (0.97,), None),               # the hparams default
    # 2048 / 2080 / 4128 / 288 samples: 1, 2, 3 and 1 de-emphasis chunks, and the restart of the chain of chunk ends
    "G": ((128, 128, 32), [65, 66, 130, 10], (2,), (0.995, 0.999), None),
    "H": ((256, 200, 50), [120, 30, 83], (2,), (0.999,), None),                # 5950 / 1450 / 4100 samples
    # 16 573 frames: 17.0 M bins and 33.9 M frame samples, both past ga_grid's clamp; three distinct utterances, every row compared
    "I": ((2048, 1200, 300), [(1000, 613, 257)[i % 3] for i in range(26)], (1,), (0.97,), 3),
    "J": ((64, 64, 16), [9, 4, 20], (0, 2), (0.97,), None),                    # the mel front: Slaney 13 x 33 basis
}
MEL_CASE = "J"
SMALL = [c for c in CASES if c != "I"]


def rows_of(name):
    """[(iters, k)] of a case"""
    _, _, iters, ks, _ = CASES[name]
    return [(it, k) for it in iters for k in ks]


def seed_of(name, iters, i):
    return 5000 + 1000 * sorted(CASES).index(name) + 100 * iters + i


def mel_setup():
    """-> (num_mels, basis (13, 33) float32, inv_basis (33, 13) float32) of case J"""
    _, hp, basis = G.mel_cases()[0]
    return hp.num_mels, basis, G.inv_basis_of(basis)


def case(name, iters, k):
    """-> (hp, [spec_i (T_i, channels)], [u_i (T_i, n_fft/2 + 1)], [(y64, y32)] per utterance, mel basis or None).  The arrays are
    read-only; utterances that repeat (case I) share their arrays and their checker runs."""
    (n_fft, win, hop), Ts, _, _, distinct = CASES[name]
    kw, channels, basis, inv = {}, None, None, None
    if name == MEL_CASE:
        channels, basis, inv = mel_setup()
        kw = {"num_mels": channels}
    hp = G.hparams(n_fft, win, hop, iters, k, **kw)
    specs, us, pairs = [], [], []
    for i, T in enumerate(Ts):
        j = i % distinct if distinct else i
        assert Ts[j] == T
        spec, u = G.inputs(n_fft, T, 1, seed_of(name, iters, j), channels=channels)
        specs.append(spec[0]); us.append(u[0])
        pairs.append(G.checkers(spec[0], u[0], hp, iters, inv, key=("ragged", name, iters, k, j)))
    return hp, specs, us, pairs, basis


def label(name, iters, k):
    (n_fft, win, hop), Ts, _, _, _ = CASES[name]
    shown = ",".join(str(t) for t in Ts) if len(Ts) <= 6 else "%d utterances of %s" % (len(Ts), sorted(set(Ts)))
    return "ragged %s n_fft %d win %d hop %d T %s iters %d k %g" % (name, n_fft, win, hop, shown, iters, k)


# the "padding is no substitute" rows: (n_fft, win, hop), frames, padded to, iterations
PADDED = [((128, 101, 25), 9, 21, 3), ((2048, 1200, 300), 9, 14, 3), ((2048, 1200, 300), 257, 1000, 1)]


def padded_then_cut(geometry, T, T_pad, iters, k=0.97):
    """-> (distance of the peak, bar of that utterance): the float64 checker on the utterance padded to T_pad frames with
    -max_abs_value (silence) and cut back to hop * (T - 1) samples, against the checker on the utterance alone"""
    n_fft, win, hop = geometry
    hp = G.hparams(n_fft, win, hop, iters, k)
    spec, u = G.inputs(n_fft, T, 1, 7000 + T + iters)
    _, u_pad = G.inputs(n_fft, T_pad - T, 1, 7500 + T + iters)
    y64, y32 = G.checkers(spec[0], u[0], hp, iters, key=("padded", geometry, T, iters, k))
    spec_p = np.concatenate([spec[0], np.full((T_pad - T, spec.shape[2]), -hp.max_abs_value, np.float32)])
    y_pad = R.inv_spectrogram(spec_p, np.concatenate([u[0], u_pad[0]]), hp, iters)[:hop * (T - 1)]
    return G.rel(y_pad, y64), G.bar(G.rel(y32, y64))
