"""-m "not gpu": the attention types of tacotron.py:127-144 at the host surface -- checkpoint tensor lists, what is refused, and the
float64 restatement tests/torch_attention_ref.py anchored to tests/torch_tacotron_ref.py."""
import numpy as np
import pytest


def _hp(**kw):
    import twvk_amd
    hp = twvk_amd.default_hparams()
    for k, v in kw.items():
        setattr(hp, k, v)
    return hp


_WANT = {   # (name, shape) after memory_layer/kernel, default sizes (attention_size = attention_state_size = 256)
    "bah_mon_norm": [("decoder/bahdanau_monotonic_attention/query_layer/kernel", (256, 256)), ("decoder/bahdanau_monotonic_attention/attention_v", (256,)),
                     ("decoder/bahdanau_monotonic_attention/attention_g", (1,)), ("decoder/bahdanau_monotonic_attention/attention_b", (256,)),
                     ("decoder/bahdanau_monotonic_attention/attention_score_bias", (1,))],
    "bah_mon": [("decoder/bahdanau_monotonic_attention/query_layer/kernel", (256, 256)), ("decoder/bahdanau_monotonic_attention/attention_v", (256,)),
                ("decoder/bahdanau_monotonic_attention/attention_score_bias", (1,))],
    "bah_norm": [("decoder/bahdanau_attention/query_layer/kernel", (256, 256)), ("decoder/bahdanau_attention/attention_v", (256,)),
                 ("decoder/bahdanau_attention/attention_g", (1,)), ("decoder/bahdanau_attention/attention_b", (256,))],
    "bah": [("decoder/bahdanau_attention/query_layer/kernel", (256, 256)), ("decoder/bahdanau_attention/attention_v", (256,))],
    "luong": [],
    "luong_scaled": [("decoder/luong_attention/attention_g", (1,))],
    "loc_sen": [("decoder/Location_Sensitive_Attention/query_layer/kernel", (256, 256)),
                ("decoder/Location_Sensitive_Attention/location_features_convolution/kernel", (31, 1, 32)),
                ("decoder/Location_Sensitive_Attention/location_features_convolution/bias", (32,)),
                ("decoder/Location_Sensitive_Attention/location_features_layer/kernel", (32, 256)),
                ("decoder/Location_Sensitive_Attention/attention_variable", (256,)),
                ("decoder/Location_Sensitive_Attention/attention_bias", (256,))],
}


@pytest.mark.parametrize("attention_type", sorted(_WANT))
def test_specs_list_the_mechanism_tensors(attention_type):
    """tacotron_specs: the mechanism's tensors replace the bahdanau_monotonic_attention block, everything else stays where it was"""
    from twvk_amd.tacotron import tacotron_specs
    base = tacotron_specs(_hp(), 2)
    specs = tacotron_specs(_hp(attention_type=attention_type), 2)
    i = [n for n, _ in base].index("memory_layer/kernel")
    assert specs[i] == ("memory_layer/kernel", (256, 256))
    got = [(n, tuple(s)) for n, s in specs[i + 1:i + 1 + len(_WANT[attention_type])]]
    assert got == _WANT[attention_type]
    assert specs[:i + 1] == base[:i + 1] and specs[i + 1 + len(_WANT[attention_type]):] == base[i + 6:]
    assert not any("attention" in n and "attention_wrapper" not in n for n, _ in specs[i + 1 + len(_WANT[attention_type]):])


def test_loc_sen_specs_follow_attention_size():
    from twvk_amd.tacotron import tacotron_specs
    sp = dict(tacotron_specs(_hp(attention_type="loc_sen", attention_size=128), 1))
    p = "decoder/Location_Sensitive_Attention/"
    assert sp[p + "query_layer/kernel"] == (256, 128) and sp[p + "location_features_layer/kernel"] == (32, 128)
    assert sp[p + "attention_variable"] == (128,) and sp["memory_layer/kernel"] == (256, 128)


@pytest.mark.parametrize("attention_type", ["luong", "luong_scaled"])
def test_luong_needs_the_query_width_of_the_keys(attention_type):
    """LuongAttention does not project the query: attention_state_size != attention_size is a graph TF cannot build"""
    from twvk_amd.tacotron import Tacotron, tacotron_specs
    hp = _hp(attention_type=attention_type, attention_size=128)
    with pytest.raises(ValueError, match="attention_state_size == attention_size"):
        tacotron_specs(hp, 2)
    with pytest.raises(ValueError):
        Tacotron(hp, num_speakers=2, device="cpu")


def test_the_c_abi_validates_attention_type():
    """twv_tacotron_create refuses unknown types and luong with a projected width of its own (host only: touches no device)"""
    import ctypes as C
    from twvk_amd import _lib
    from twvk_amd.tacotron import Tacotron
    m = Tacotron(_hp(attention_type="bah"), num_speakers=2, device="cpu")
    L = _lib.lib()
    d = _lib.TacoDims.from_buffer_copy(m._dims)
    assert d.attention_type == 3
    for at, A in ((7, 256), (-1, 256), (4, 128), (5, 128)):
        e = _lib.TacoDims.from_buffer_copy(d)
        e.attention_type, e.attention_size = at, A
        h = C.c_void_p()
        assert L.twv_tacotron_create(C.byref(e), C.byref(h)) == 1, (at, A)          # TWV_E_INVALID
    for at in range(7):
        e = _lib.TacoDims.from_buffer_copy(d)
        e.attention_type = at
        h = C.c_void_p()
        assert L.twv_tacotron_create(C.byref(e), C.byref(h)) == 0, at
        L.twv_tacotron_destroy(h)


@pytest.mark.parametrize("attention_type", ["gmm", "bah_mon_norm_hccho", "no_such_type"])
def test_unbuilt_attention_types_still_raise(attention_type):
    from twvk_amd.tacotron import Tacotron
    with pytest.raises(NotImplementedError) as e:
        Tacotron(_hp(attention_type=attention_type), num_speakers=2, device="cpu")
    for t in ("bah_mon_norm", "bah_mon", "bah_norm", "bah", "luong", "luong_scaled", "loc_sen"):
        assert "'%s'" % t in str(e.value) or t in str(e.value)


@pytest.mark.parametrize("attention_type", ["bah_mon_norm", "bah", "loc_sen"])
def test_blob_size_follows_the_specs(attention_type):
    from twvk_amd.tacotron import Tacotron, flatten
    import torch_attention_ref as AR
    m = Tacotron(_hp(attention_type=attention_type), num_speakers=2, device="cpu")
    blob = flatten(m.specs, AR.random_tensors(m.specs, 3))
    assert blob.size == m._L.twv_tacotron_blob_floats(m._h)


@pytest.mark.parametrize("num_speakers", [1, 2])
def test_restatement_bah_mon_norm_mode_is_the_tacotron_restatement(num_speakers):
    """torch_attention_ref in 'bah_mon_norm' mode == torch_tacotron_ref.infer, bit for bit (the latter is cross-checked against oracle/)"""
    import torch_attention_ref as AR
    import torch_tacotron_ref as R
    from twvk_amd.tacotron import tacotron_specs
    hp = _hp(max_iters=5, enc_bank_size=3, post_bank_size=2, num_freq=65)
    specs = tacotron_specs(hp, num_speakers)
    w = AR.random_tensors(specs, 11)
    rng = np.random.RandomState(12)
    N, T, lengths = 3, 17, [17, 9, 4]
    tok = rng.randint(2, 80, (N, T)).astype(np.int32)
    for n, ln in enumerate(lengths):
        tok[n, ln - 1] = 1
        tok[n, ln:] = 0
    spk = np.array([1, 0, 1], np.int32) if num_speakers > 1 else None
    dims = AR.Dims(hp, num_speakers)
    a = AR.infer(w, dims, tok, np.asarray(lengths), spk, "bah_mon_norm")
    b = R.infer(w, dims, tok, np.asarray(lengths), spk)
    for x, y in zip(a, b):
        assert x.shape == y.shape and np.array_equal(x, y)


@pytest.mark.parametrize("attention_type", ["bah_mon", "bah_norm", "bah", "luong", "luong_scaled", "loc_sen"])
def test_restatement_softmax_and_state(attention_type):
    """the restatement's own invariants: softmax alignments sum to 1 over the valid positions and are 0 past them; the types differ"""
    import torch_attention_ref as AR
    from twvk_amd.tacotron import tacotron_specs
    hp = _hp(max_iters=4, enc_bank_size=2, post_bank_size=2, num_freq=33, attention_type=attention_type)
    specs = tacotron_specs(hp, 2)
    w = AR.random_tensors(specs, 5)
    rng = np.random.RandomState(6)
    N, T, lengths = 2, 13, [13, 6]
    tok = rng.randint(2, 80, (N, T)).astype(np.int32)
    tok[1, 5] = 1; tok[1, 6:] = 0
    mel, lin, al = AR.infer(w, AR.Dims(hp, 2), tok, np.asarray(lengths), np.array([0, 1]), attention_type)
    assert np.isfinite(mel).all() and np.isfinite(lin).all()
    assert np.all(al[1, 6:] == 0)
    if attention_type != "bah_mon":
        assert np.allclose(al[0].sum(axis=0), 1.0, atol=1e-12) and np.allclose(al[1, :6].sum(axis=0), 1.0, atol=1e-12)
