"""-m "not gpu": the host side of train_tacotron -- the initial values of TacotronTrainer.init_weights by distribution, and
the command line's argument and directory rules."""
import json
import os
import types

import numpy as np
import pytest

from tacotron_grad_cases import SMALL, hparams


# ---------------------------------------------------------------- init_weights
def _specs(speakers=2, **kw):
    from twvk_amd.tacotron import tacotron_specs
    hp = hparams(max_iters=8, **dict(SMALL, **kw))
    return hp, tacotron_specs(hp, speakers)


def test_initial_tensors_have_every_tensor_and_the_reference_constants():
    from twvk_amd.tacotron_train import glorot_limit, initial_tensors, initializer_of
    hp, specs = _specs()
    t = initial_tensors(specs, hp, seed=3)
    assert list(t) == [n for n, _ in specs]
    for n, shp in specs:
        assert t[n].shape == tuple(shp) and t[n].dtype == np.float32, n
    A = hp.attention_size
    p = "decoder/bahdanau_monotonic_attention/"
    assert np.array_equal(t[p + "attention_g"], np.full(1, np.sqrt(1.0 / A), np.float32))
    assert not t[p + "attention_b"].any() and not t[p + "attention_score_bias"].any()
    seen = {"gates": 0, "candidate": 0, "T": 0, "bn": 0, "bias": 0, "kernel": 0}
    for n, shp in specs:
        if n.endswith("batch_normalization"):
            C_ = shp[1]
            assert np.array_equal(t[n], np.stack([np.ones(C_), np.zeros(C_), np.zeros(C_), np.ones(C_)]).astype(np.float32)), n
            seen["bn"] += 1
        elif n.endswith("gates/bias"):
            assert np.array_equal(t[n], np.ones(shp, np.float32)), n
            seen["gates"] += 1
        elif n.endswith("candidate/bias"):
            assert not t[n].any(), n
            seen["candidate"] += 1
        elif n.endswith("/T/bias"):
            assert np.array_equal(t[n], np.full(shp, -1.0, np.float32)), n
            seen["T"] += 1
        elif n.endswith("/bias"):
            assert not t[n].any(), n
            seen["bias"] += 1
        elif n.endswith("/kernel") or n.endswith("attention_v"):
            lim = glorot_limit(shp)
            assert initializer_of(n, shp) == ("glorot_uniform", lim)
            assert float(np.abs(t[n]).max()) <= np.float32(lim) and t[n].any(), n
            seen["kernel"] += 1
    # 7 GRUs (2 x 2 bidirectional, the attention cell, 2 decoder layers), 8 highway layers, (4 + 2) + (3 + 2) batch norms
    assert seen["gates"] == seen["candidate"] == 7 and seen["T"] == 8 and seen["bn"] == 11 and seen["bias"] > 20 and seen["kernel"] > 40, seen
    # the bounds: a dense kernel (in, out), a conv1d kernel (taps, in, out) with fan = taps x channels, a vector
    assert glorot_limit((256, 128)) == pytest.approx(np.sqrt(6.0 / 384)) and glorot_limit((3, 128, 64)) == pytest.approx(np.sqrt(6.0 / (3 * 192)))
    assert glorot_limit((256,)) == pytest.approx(np.sqrt(6.0 / 512))
    # truncated normal: nothing beyond two standard deviations
    assert float(np.abs(t["embedding"]).max()) <= 1.0 and float(np.abs(t["speaker_embedding"]).max()) <= 1.0
    assert float(np.abs(t["embedding"]).max()) > 0.9                       # (20480 draws reach the edge)


def test_sample_variances_and_seeds():
    from twvk_amd.tacotron_train import TRUNCATED_VARIANCE, glorot_limit, initial_tensors
    hp, specs = _specs()
    t = initial_tensors(specs, hp, seed=3)
    # the variance of a unit normal cut at 2: 1 - 2 * 2 * pdf(2) / (cdf(2) - cdf(-2))
    from math import erf, exp, pi, sqrt
    assert TRUNCATED_VARIANCE == pytest.approx(1.0 - 4.0 * exp(-2.0) / sqrt(2.0 * pi) / erf(2.0 / sqrt(2.0)), abs=1e-6)
    big = [(n, shp) for n, shp in specs if int(np.prod(shp)) >= 16384 and not n.endswith("batch_normalization")]
    assert len(big) >= 20 and "embedding" in dict(big)
    for n, shp in big:
        a = t[n].astype(np.float64)
        want = 0.25 * TRUNCATED_VARIANCE if n == "embedding" else glorot_limit(shp) ** 2 / 3.0
        assert abs(a.var() / want - 1.0) <= 0.05, (n, a.var(), want)
        assert abs(a.mean()) <= 5.0 * np.sqrt(want / a.size), n
    again, other = initial_tensors(specs, hp, seed=3), initial_tensors(specs, hp, seed=4)
    assert all(np.array_equal(t[n].view(np.uint32), again[n].view(np.uint32)) for n in t)
    assert not np.array_equal(t["embedding"], other["embedding"])


def test_the_tables_of_speaker_embedding_size_one_and_other_attentions():
    from twvk_amd.tacotron_train import initial_tensors, initializer_of
    hp, specs = _specs(speaker_embedding_size=1)
    t = initial_tensors(specs, hp, seed=0)
    tables = ["before_highway", "encoder_rnn_init_state", "attention_rnn_init_state", "decoder_rnn_init_states1", "decoder_rnn_init_states2"]
    assert all(n in t for n in tables) and "speaker_embedding" not in t
    for n in tables:
        assert initializer_of(n, t[n].shape) == ("truncated_normal", 0.1) and float(np.abs(t[n]).max()) <= np.float32(0.2) and t[n].any()
    hp, specs = _specs(speakers=1, attention_type="luong_scaled", attention_size=256)
    t = initial_tensors(specs, hp, seed=0)
    assert np.array_equal(t["decoder/luong_attention/attention_g"], np.ones(1, np.float32)) and "speaker_embedding" not in t
    hp, specs = _specs(speakers=1, attention_type="loc_sen")
    t = initial_tensors(specs, hp, seed=0)
    p = "decoder/Location_Sensitive_Attention/"
    assert t[p + "attention_variable"].any() and not t[p + "attention_bias"].any() and not t[p + "location_features_convolution/bias"].any()


# ---------------------------------------------------------------- the command line
def test_argument_rules():
    from twvk_amd.train_tacotron import get_arguments
    c = get_arguments(["--data_paths", "a/x,b/y"])
    assert c.data_paths == ["a/x", "b/y"] and (c.log_dir, c.load_path, c.initialize_path) == ("logdir-tacotron", None, None)
    assert (c.batch_size, c.num_test_per_speaker, c.random_seed, c.summary_interval, c.test_interval, c.checkpoint_interval) == (32, 2, 123, 100000, 500, 2000)
    assert c.skip_path_filter is False and c.training is True and c.num_steps is None
    c = get_arguments(["--skip_path_filter", "true", "--training", "false", "--num_steps", "7", "--slack_url", "u", "--git"])
    assert c.skip_path_filter is True and c.training is False and c.num_steps == 7
    with pytest.raises(ValueError, match="Only one of load_path and initialize_path"):
        get_arguments(["--load_path", "a", "--initialize_path", "b"])


def test_directories_are_decided_once_and_params_are_written(tmp_path):
    from twvk_amd.train_tacotron import get_arguments, prepare_dirs
    hp = hparams(max_iters=8, **SMALL)
    calls = []

    def now():
        calls.append(1)
        return "2025-01-02_03-04-0%d" % len(calls)
    c = get_arguments(["--log_dir", str(tmp_path / "logs"), "--data_paths", "%s,%s" % (tmp_path / "data" / "moon", tmp_path / "data" / "son")])
    model_dir = prepare_dirs(c, hp, now)
    assert calls == [1] and model_dir == str(tmp_path / "logs" / "moon+son_2025-01-02_03-04-01") and os.path.isdir(model_dir)
    params = json.load(open(os.path.join(model_dir, "params.json"), encoding="utf-8"))
    assert params["num_speakers"] == 2 and params["max_iters"] == 8 and params["num_freq"] == 129
    # --load_path: that directory, its params.json over the hyper-parameters, nothing new made
    other = hparams(max_iters=200)
    c = get_arguments(["--log_dir", str(tmp_path / "logs"), "--load_path", model_dir, "--data_paths", "x/moon,x/son"])
    assert prepare_dirs(c, other, now) == model_dir and calls == [1]
    assert other.max_iters == 8 and other.num_freq == 129 and sorted(os.listdir(str(tmp_path / "logs"))) == ["moon+son_2025-01-02_03-04-01"]


def test_initialize_path_resets_the_step_and_load_path_keeps_it():
    from twvk_amd.train_tacotron import start_state
    seen = []

    def trainer():
        t = types.SimpleNamespace(global_step=0)

        def restore(path, verify=False):
            seen.append((path, verify))
            t.global_step = 41
            return 41
        t.restore = restore
        return t
    quiet = lambda *a: None
    cfg = lambda **kw: types.SimpleNamespace(**dict(dict(load_path=None, initialize_path=None), **kw))
    t = trainer()
    assert start_state(cfg(load_path="run"), t, "run", quiet) == 41 == t.global_step
    t = trainer()
    assert start_state(cfg(initialize_path="other"), t, "new", quiet) == 0 == t.global_step
    t = trainer()
    assert start_state(cfg(), t, "new", quiet) == 0
    assert seen == [("run", True), ("other", True)]


def test_value_window():
    from twvk_amd.train_tacotron import ValueWindow
    w = ValueWindow(3)
    assert w.average == 0
    for x in (1.0, 2.0, 3.0, 10.0):
        w.append(x)
    assert w.average == pytest.approx(5.0)
