"""Host-only side of generation at residual / dilation widths 64 and 128: layouts, sizes, names and refusals (no device is touched)."""
import ctypes as C
import subprocess

import numpy as np
import pytest

WIDTHS = [(64, 64), (128, 128), (32, 64), (64, 32), (128, 64)]
DIL = [1, 2, 4, 8]


def _dims(_lib, d, R, D):
    dims = _lib.Dims()
    dims.n_layers = len(DIL)
    for i, v in enumerate(DIL):
        dims.dilations[i] = v
    dims.residual_channels, dims.dilation_channels = R, D
    dims.skip_channels, dims.quantization_channels, dims.out_channels = d.S, d.Q, 30
    dims.scalar_input, dims.initial_filter_width, dims.use_biases = d.scalar_input, 32, d.use_bias
    dims.gc_channels, dims.gc_cardinality, dims.lc_channels = d.G, d.gc_card, d.L
    dims.n_upsample = 3 if d.L else 0
    for i, v in enumerate((5, 5, 12)):
        dims.upsample_factor[i] = v
    return dims


@pytest.mark.parametrize("kw", [dict(), dict(scalar_input=False), dict(use_bias=False, G=0)])
@pytest.mark.parametrize("R,D", WIDTHS)
def test_wide_host_calls_agree_with_oracle(oracle, R, D, kw):
    import twvk_amd  # noqa: F401
    from twvk_amd import weights as W, _lib
    d = oracle.make_dims(DIL, R=R, D=D, **kw)
    tensors = oracle.random_tensors(d, seed=1)
    specs = W.tensor_specs(len(DIL), R, D, d.S, d.Q, 30, bool(d.scalar_input), 32, bool(d.use_bias), d.G, d.gc_card, d.L, (5, 5, 12))
    assert [n for n, _ in specs] == [n for n, _ in oracle.tensor_specs(d)]
    assert np.array_equal(W.flatten(specs, tensors), oracle.blob_from_tensors(d, tensors))
    L = _lib.lib()
    h = C.c_void_p()
    _lib.check(L.twv_wavenet_create(C.byref(_dims(_lib, d, R, D)), C.byref(h)))      # host-only: no device is touched
    try:
        assert L.twv_wavenet_blob_floats(h) == oracle.blob_floats(d)
        assert L.twv_wavenet_receptive_field(h) == oracle.receptive_field(d)
        assert L.twv_wavenet_hop_size(h) == 300
        assert L.twv_wavenet_packed_bytes(h) > 0
        assert L.twv_wavenet_state_bytes(h, 3) > 0
        assert L.twv_wavenet_cond_bytes(h, 3, 10) > 0
        assert L.twv_wavenet_cond_bytes(h, 3, 11) - L.twv_wavenet_cond_bytes(h, 3, 10) == 3 * len(DIL) * 2 * D * 4
        name = L.twv_wavenet_kernel_name(h, 3)
        assert (name.decode() if isinstance(name, bytes) else name) == "wn_wide_generate_kernel"
        assert L.twv_wavenet_fused_conditioning(h, 3) == 0
        # the launch-geometry options of the other kernels are accepted and change nothing
        before = (L.twv_wavenet_state_bytes(h, 3), L.twv_wavenet_cond_bytes(h, 3, 10))
        for name_, v in ((b"xcd", 0), (b"xcd_many", 1), (b"helpers", 0), (b"workers", 3), (b"groups", 2)):
            _lib.check(L.twv_wavenet_set_option(h, name_, v))
        assert (L.twv_wavenet_state_bytes(h, 3), L.twv_wavenet_cond_bytes(h, 3, 10)) == before
        name = L.twv_wavenet_kernel_name(h, 3)
        assert (name.decode() if isinstance(name, bytes) else name) == "wn_wide_generate_kernel"
    finally:
        L.twv_wavenet_destroy(h)


def test_width_32_keeps_its_kernels():
    import twvk_amd  # noqa: F401
    from twvk_amd.wavenet import WaveNetModel
    m = WaveNetModel(1, DIL, 2, 32, 32, 512, scalar_input=True, out_channels=30, local_condition_channels=None, device="cpu")
    name = m._L.twv_wavenet_kernel_name(m._h, 1)
    assert (name.decode() if isinstance(name, bytes) else name) in ("wn_generate_kernel", "wn_xcd_generate_kernel")


@pytest.mark.parametrize("bad", [16, 48, 96, 256])
def test_other_widths_are_refused_with_the_accepted_set(bad):
    import twvk_amd  # noqa: F401
    from twvk_amd.wavenet import WaveNetModel
    from twvk_amd._lib import TwvError
    for R, D in ((bad, 64), (64, bad), (bad, bad)):
        with pytest.raises(TwvError) as e:
            WaveNetModel(1, [1, 2], 2, R, D, 512, scalar_input=True, out_channels=30, device="cpu")
        assert all(s in str(e.value) for s in ("32", "64", "128")), str(e.value)


@pytest.mark.parametrize("R,D", [(64, 64), (128, 32)])
def test_training_on_a_wide_model_is_refused(R, D):
    import twvk_amd  # noqa: F401
    from twvk_amd import _lib
    from twvk_amd.wavenet import WaveNetModel
    m = WaveNetModel(2, DIL, 2, R, D, 512, scalar_input=True, out_channels=30, use_biases=True, global_condition_channels=32,
                     global_condition_cardinality=2, local_condition_channels=80, upsample_factor=[5, 5, 12], device="cpu")
    L = _lib.lib()
    h = C.c_void_p()
    with pytest.raises(_lib.TwvError, match="training at other widths is not built"):
        _lib.check(L.twv_wavenet_train_create(C.byref(m._dims), 2, 1200, C.byref(h)))
    assert not h.value


def test_wide_kernel_is_in_the_library():
    import twvk_amd  # noqa: F401
    from twvk_amd import _lib
    nm = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    assert "wn_wide_generate_kernel" in nm, "the gfx950 wide generation kernel must be in the library"
