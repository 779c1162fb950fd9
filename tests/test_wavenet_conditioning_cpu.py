"""Host-only side of tests/conditioning_cases.py (the oracle alone, and the library's host calls: no device is touched).

1. The inputs of every row discriminate in the channels and taps the row's shape adds.  After the conditions of
   tests/sensitive_inputs.py are asserted on the oracle's output, ONE slice of one conditioning tensor is scaled by float32(1 + 2^-10)
   -- the last input channel of lc_filter / lc_gate / gc_filter / gc_gate of the first and of the last layer, the last tap of every
   upsampling kernel, the last row and last column of gc_embedding -- and the oracle, on the SAME inputs, must draw at least one other
   sample; the median mutant must move a quarter of them (the bar of test_every_mutant_is_killed; measured: the median moves more
   than eight samples in ten, the weakest mutant 39 of 180).
   A kernel that drops, zeroes or misplaces such a channel therefore cannot pass tests/test_wavenet_conditioning_gpu.py.
   The one survivor found while writing this: the last tap of upsample0 when T ends before that tap's phase ((5, 5, 12): T < 241),
   which is why conditioning_cases.steps covers every phase of every stage.
2. Which generation kernel the library takes for the rows at the edges of the many-streams kernel's LDS bound.  The model's
   kernel_name() / fused_conditioning() enter the device's context, so the C calls behind them are asked here; the GPU file asserts
   the same through the model before every run.
3. What twv_wavenet_create refuses: an error status, a message, no handle."""
import ctypes as C

import numpy as np
import pytest

import conditioning_cases as CC
import sensitive_inputs as SI


@pytest.mark.parametrize("rid", list(CC.ROWS))
def test_single_channel_mutants_are_killed(oracle, rid):
    B = 3
    c = CC.case(oracle, rid, B)                     # (helpers.sensitive_mol has asserted the conditions; once more, with the figures)
    SI.assert_mol_inputs(c.u, c.want, int(round(c.figures()[1] * B * c.T)))
    assert c.T >= 2 * CC.hop(rid) + 3 and c.mel.shape[1] * CC.hop(rid) >= c.T + CC.hop(rid)
    rows = [(label,) + SI.changed_samples(CC.rerun(oracle, c, t), c.want) for label, t in CC.channel_mutants(c)]
    print(rid, "T", c.T, "clamp share %.3f edge share %.3f" % c.figures(), [(label.replace("wavenet/", ""), n) for label, n, _ in rows])
    assert len(rows) == 8 + c.d.n_up + (2 if c.kw["gc_card"] else 0)
    assert CC.rerun(oracle, c, c.tensors).tobytes() == c.want.tobytes()          # rerun itself moves nothing
    survivors = [label for label, n, _ in rows if n == 0]
    assert not survivors, "mutants that change no sample: %s" % survivors
    killed = sorted(n for _, n, _ in rows)
    assert killed[len(killed) // 2] >= (B * c.T) // 4, killed


def _host_model(rid, B, **options):
    import twvk_amd  # noqa: F401
    from twvk_amd.wavenet import WaveNetModel
    g = CC.geometry(rid)
    m = WaveNetModel(B, CC.dilations(), 2, 32, 32, 512, out_channels=30, use_biases=True, scalar_input=True,
                     global_condition_channels=g["G"], global_condition_cardinality=g["gc_card"] or None,
                     local_condition_channels=g["L"], upsample_factor=list(g["up"]), train_mode=False, device="cpu")
    for k, v in options.items():
        m.set_option(k, v)
    return m


@pytest.mark.parametrize("rid,B,options,kernel,fused", [("l36", 40, {}, "wn_xcd_many_kernel", 1),
                                                        ("l100", 40, {}, "wn_xcd_many_kernel", 1),
                                                        ("l100", 9, dict(xcd_many=1), "wn_xcd_many_kernel", 1),
                                                        ("l128", 9, dict(xcd_many=1), "wn_xcd_generate_kernel", 1),
                                                        ("l128", 32, {}, "wn_xcd_generate_kernel", 1),
                                                        ("l128", 33, {}, "wn_generate_kernel", 0),
                                                        ("l128", 3, dict(xcd=0), "wn_generate_kernel", 0)])
def test_kernel_choice_at_the_many_streams_lds_bound(rid, B, options, kernel, fused):
    """(n_up + 1) * NLC: l36 10, l100 12 (the bound), l128 20 -- there `xcd_many` = 1 is ignored and batches above 32 go to the generic
    kernel.  Without a device the library assumes the MI355X's 256 CUs."""
    m = _host_model(rid, B, **options)
    assert m._L.twv_wavenet_kernel_name(m._h, B).decode() == kernel
    assert m._L.twv_wavenet_fused_conditioning(m._h, B) == fused
    assert m.hop_size == CC.hop(rid)


REFUSED = [("lc_channels 2", dict(L=2)), ("lc_channels 82", dict(L=82)), ("lc_channels 132", dict(L=132)),
           ("gc_channels 65", dict(G=65)), ("n_upsample 0", dict(up=())), ("n_upsample 5", dict(up=(2, 2, 2, 2, 2))),
           ("a factor of 0", dict(up=(5, 0, 12)))]


@pytest.mark.parametrize("what,kw", REFUSED, ids=[r[0] for r in REFUSED])
def test_create_refuses(what, kw):
    import twvk_amd  # noqa: F401
    from twvk_amd import _lib
    from twvk_amd.wavenet import WaveNetModel
    g = dict(L=80, up=(5, 5, 12), G=32)
    g.update(kw)
    with pytest.raises(_lib.TwvError) as e:             # the model hands every one of these values on to the library
        WaveNetModel(1, CC.dilations(), 2, 32, 32, 512, out_channels=30, use_biases=True, scalar_input=True,
                     global_condition_channels=g["G"], global_condition_cardinality=2, local_condition_channels=g["L"],
                     upsample_factor=list(g["up"]), train_mode=False, device="cpu")
    assert len(str(e.value)) > len("twv_amd error 0: ")
    # the C-ABI itself: an error status, a message, no handle
    d = _lib.Dims()
    dil = CC.dilations()
    d.n_layers = len(dil)
    for i, v in enumerate(dil):
        d.dilations[i] = v
    d.residual_channels, d.dilation_channels, d.skip_channels, d.quantization_channels, d.out_channels = 32, 32, 512, 256, 30
    d.scalar_input, d.initial_filter_width, d.use_biases = 1, 32, 1
    d.gc_channels, d.gc_cardinality, d.lc_channels, d.n_upsample = g["G"], 2, g["L"], len(g["up"])
    for i, v in enumerate(g["up"][:4]):
        d.upsample_factor[i] = v
    L = _lib.lib()
    h = C.c_void_p()
    rc = L.twv_wavenet_create(C.byref(d), C.byref(h))
    assert rc != 0 and not h.value, (what, rc, h.value)
    assert L.twv_last_error().decode().strip(), what
    # ... and the neighbouring accepted value is taken: the refusal is about this value
    ok = dict(L=80, up=(5, 5, 12), G=32)
    ok.update({"lc_channels 2": dict(L=4), "lc_channels 82": dict(L=84), "lc_channels 132": dict(L=128), "gc_channels 65": dict(G=64),
               "n_upsample 0": dict(up=(300,)), "n_upsample 5": dict(up=(2, 2, 2, 2)), "a factor of 0": dict(up=(5, 1, 12))}[what])
    d.gc_channels, d.lc_channels, d.n_upsample = ok["G"], ok["L"], len(ok["up"])
    for i, v in enumerate(ok["up"]):
        d.upsample_factor[i] = v
    _lib.check(L.twv_wavenet_create(C.byref(d), C.byref(h)))
    assert h.value
    L.twv_wavenet_destroy(h)


def test_table_reaches_the_arms_it_names():
    """the numbers the kernels branch on, as plain arithmetic on the table: an edit of a row cannot quietly lose an arm"""
    nlc = {r: (CC.geometry(r)["L"] + 31) // 32 for r in CC.ROWS}
    assert [nlc[r] for r in CC.L_ROWS] == [1, 1, 1, 2, 2, 3, 3, 4, 4]
    assert sorted(len(CC.geometry(r)["up"]) for r in CC.L_ROWS) == [1, 2, 2, 2, 2, 3, 3, 4, 4]
    assert 1 in CC.geometry("l32f1")["up"]
    assert [CC.steps(r) for r in CC.L_ROWS] == [60, 60, 60, 123, 60, 603, 603, 60, 60] and {CC.steps(r) for r in CC.G_ROWS} == {603}
    assert [CC.geometry(r)["G"] for r in CC.G_ROWS] == [1, 5, 33, 64, 48] and CC.geometry("g48emb")["gc_card"] == 0
    assert np.prod(CC.geometry("l68")["up"]) == 300 and CC.dilations(9) == CC.DIL7 + [1, 2]
