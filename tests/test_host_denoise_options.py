"""The denoise loop's options, the parts that need no device: fmi_flux_denoise_with is declared, exported and bound, the ctypes mirror of
fmi_flux_denoise_options has the header's fields in the header's order, and a null handle is refused — through the new entry and through each older one, which
are the same path — before anything is touched."""
import ctypes as C
import os
import re

from diffusion_rs_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEGACY = {"fmi_flux_denoise": 6, "fmi_flux_denoise_inpaint": 9, "fmi_flux_denoise_context": 10, "fmi_flux_denoise_cached": 11, "fmi_flux_denoise_cfg": 11,
          "fmi_flux_denoise_control": 11}


def _header_code():
    hdr = open(os.path.join(ROOT, "include", "flux_mi355x.h")).read()
    return re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)


def test_the_entry_is_declared_exported_and_bound_next_to_the_older_ones():
    code, lib = _header_code(), L.load()
    for s, nargs in dict(LEGACY, fmi_flux_denoise_with=7).items():
        assert s in L.EXPORTED
        assert re.search(r"\bint\s+" + s + r"\s*\(", code), s
        assert hasattr(lib, s) and len(getattr(lib, s).argtypes) == nargs, s
    a = lib.fmi_flux_denoise_with.argtypes
    assert a == [C.c_void_p, C.POINTER(L.FluxInputs), C.POINTER(L.FluxDenoiseOptions), C.c_void_p, C.POINTER(C.c_double), C.c_int, C.c_void_p]
    assert lib.fmi_abi_version() == 6


def test_the_options_mirror_has_the_headers_fields_in_the_headers_order():
    body = re.search(r"typedef\s+struct\s+fmi_flux_denoise_options\s*\{(.*?)\}\s*fmi_flux_denoise_options\s*;", _header_code(), flags=re.S).group(1)
    names = []
    for decl in body.split(";"):  # `const T* a` or `const float *x0, *noise, *mask`: the declarators are what follows each `*`
        names += [d.strip() for d in re.findall(r"\*\s*(\w+)", decl)]
    assert names == ["ctx", "ctl", "cfg", "cache", "x0", "noise", "mask"]
    T = L.FluxDenoiseOptions
    assert [f[0] for f in T._fields_] == names
    # seven pointers, no padding
    assert [getattr(T, n).offset for n in names] == [8 * i for i in range(7)] and C.sizeof(T) == 56
    assert [f[1] for f in T._fields_[:4]] == [C.POINTER(L.FluxContext), C.POINTER(L.FluxControl), C.POINTER(L.FluxTrueCfg), C.POINTER(L.FluxStepCache)]
    o = T()  # a fresh struct is all NULL: the options-free loop
    assert not any((o.ctx, o.ctl, o.cfg, o.cache)) and (o.x0, o.noise, o.mask) == (None, None, None)


def test_a_null_handle_is_refused_by_every_entry():
    lib = L.load()
    inp, opts, buf, ts = L.FluxInputs(), L.FluxDenoiseOptions(), (C.c_float * 8)(), (C.c_double * 2)(1.0, 0.0)
    assert lib.fmi_flux_denoise_with(None, None, None, None, None, 0, None) == L.ERR_INVALID
    assert lib.fmi_flux_denoise_with(None, C.byref(inp), C.byref(opts), buf, ts, 1, None) == L.ERR_INVALID
    assert len(lib.fmi_last_error()) > 0
    # x0 / noise / mask in part is refused on its own account, handle or no handle
    opts.x0 = C.cast(buf, C.c_void_p)
    assert lib.fmi_flux_denoise_with(None, C.byref(inp), C.byref(opts), buf, ts, 1, None) == L.ERR_INVALID
    assert b"go together" in lib.fmi_last_error()
    for s in LEGACY:
        assert getattr(lib, s)(*[0 if t == C.c_int else None for t in getattr(lib, s).argtypes]) == L.ERR_INVALID, s


# ------------------------------------------------------------------------------------------------ which options combine: Python's one table
# the header's table at fmi_flux_denoise_with, written out: the eight pairs of options that are refused, and the modes an option does not run in
OPTIONS = ("context", "control", "true_cfg", "cache", "blend", "controlnet", "ip_adapter")
PAIRS = [("control", "context"), ("control", "cache"), ("true_cfg", "cache"), ("controlnet", "context"), ("controlnet", "control"), ("controlnet", "cache"),
         ("ip_adapter", "context"), ("ip_adapter", "cache")]
MODES = [("cache", "sequence_parallel"), ("true_cfg", "sequence_parallel"), ("control", "sequence_parallel"), ("controlnet", "sequence_parallel"),
         ("ip_adapter", "sequence_parallel"), ("ip_adapter", "fp8"), ("ip_adapter", "int8")]


def test_the_table_holds_the_headers_eight_pairs_and_the_seven_mode_rows():
    from diffusion_rs_amd import flux as F
    assert len(F.REFUSED_PAIRS) == 8 and {frozenset(r) for r in F.REFUSED_PAIRS} == {frozenset(p) for p in PAIRS}
    assert len(F.REFUSED_MODES) == 7 and set(F.REFUSED_MODES) == set(MODES)
    # the header says the same of the struct's own fields: the three FMI_ERR_UNSUPPORTED cells of its grid
    grid = re.search(r"Which options combine.*?\n(.*?)\(cn:", open(os.path.join(ROOT, "include", "flux_mi355x.h")).read(), flags=re.S).group(1)
    assert grid.count("FMI_ERR_UNSUPPORTED") == 3 + 3  # ctx x ctl, ctl x cache, cfg x cache; and the cn row's ctx, ctl, cache


def test_every_subset_of_the_options_is_refused_iff_it_holds_a_refused_pair():
    import pytest
    from diffusion_rs_amd import flux as F
    from diffusion_rs_amd import pipeline as pl
    for names in (F.OPTION_NAMES, pl.REQUEST_NAMES):
        for bits in range(1 << len(OPTIONS)):
            present = {o for i, o in enumerate(OPTIONS) if bits >> i & 1}
            if any(set(p) <= present for p in PAIRS):
                with pytest.raises(ValueError, match="is not combined with"):
                    F.check_combination(present, names)
            else:
                assert F.check_combination(present, names) is None
        for mode in ("sequence_parallel", "fp8", "int8"):
            for o in OPTIONS:
                if (o, mode) in MODES:
                    with pytest.raises(ValueError, match="sequence parallelism" if mode == "sequence_parallel" else mode + " mode"):
                        F.check_combination({o, mode}, names)
                else:
                    assert F.check_combination({o, mode}, names) is None


def _flux_call_kw(torch, F, option):
    """FluxModel.denoise's keywords that make `option` present, for img (1,4,64), txt (1,2,J), y (1,P) on the host"""
    from tests.util import SMALL_FLUX
    if option == "context":
        return dict(context=torch.zeros(1, 3, 64), context_ids=torch.zeros(1, 3, 3))
    if option == "control":
        return dict(control=torch.zeros(1, 4, 64))
    if option == "true_cfg":
        return dict(negative_txt=torch.zeros(1, 2, SMALL_FLUX["joint_attention_dim"]), negative_y=torch.zeros(1, SMALL_FLUX["pooled_projection_dim"]))
    if option == "cache":
        return dict(cache_threshold=0.1)
    if option == "controlnet":
        net = object.__new__(F.FluxControlNetModel)  # no device: a refused call never reaches its handle
        net.cfg, net.h = dict(SMALL_FLUX, num_layers=1, num_single_layers=1), None
        return dict(controlnet=net, controlnet_cond=torch.zeros(1, 4, 64))
    assert option == "ip_adapter"
    ada = object.__new__(F.FluxIPAdapter)
    ada.h, ada.dims = None, dict(num_heads=SMALL_FLUX["num_attention_heads"], joint_attention_dim=SMALL_FLUX["joint_attention_dim"], num_layers=SMALL_FLUX["num_layers"],
                    embed_dim=16, num_tokens=4)
    return dict(ip_adapter=ada, ip_adapter_image_embeds=torch.zeros(1, 16))


def test_flux_model_refuses_each_row_before_any_library_call():
    """a FluxModel without a handle or a library: a call that got past the Python checks would fail on the missing attribute, not with ValueError"""
    import pytest
    import torch
    from diffusion_rs_amd import flux as F
    from tests.util import SMALL_FLUX

    def model(conditioned, mode=None):
        m = object.__new__(F.FluxModel)
        m.cfg, m.state_channels, m.cond_channels = dict(SMALL_FLUX), 64, 64 if conditioned else 0
        if mode == "sequence_parallel":
            m._sp_world = 2
        elif mode:
            m._eight_bit = mode
        return m

    img, ids, txt, txt_ids = torch.zeros(1, 4, 64), torch.zeros(1, 4, 3), torch.zeros(1, 2, SMALL_FLUX["joint_attention_dim"]), torch.zeros(1, 2, 3)
    y, g = torch.zeros(1, SMALL_FLUX["pooled_projection_dim"]), torch.zeros(1)
    for a, b in PAIRS + MODES:
        kw = dict(_flux_call_kw(torch, F, a), **({} if b in ("sequence_parallel", "fp8", "int8") else _flux_call_kw(torch, F, b)))
        m = model("control" in (a, b), b)
        match = "is not combined with" if (a, b) in PAIRS else ("sequence parallelism" if b == "sequence_parallel" else b + " mode")
        with pytest.raises(ValueError, match=match):
            m.denoise(img, ids, txt, txt_ids, y, g, [1.0, 0.5, 0.0], **kw)
        if not {a, b} & {"true_cfg", "cache"}:  # forward has neither
            with pytest.raises(ValueError, match=match):
                m.forward(img, ids, txt, txt_ids, torch.zeros(1), y, g, **kw)


def test_pipeline_refuses_each_row_before_any_chunk():
    import pytest
    import torch
    from diffusion_rs_amd import pipeline as pl
    H = W = 16

    class _Flux:
        cond_channels = 0

    class _Adapter:
        embed_dim = 16

    class RecordingPipeline(pl.Pipeline):
        def __init__(self):  # no GPU: only the request path in front of the chunk body is under test
            self.device, self.flux, self.controlnet, self.ip_adapter, self.calls = torch.device("cpu"), _Flux(), object(), _Adapter(), []

        def _generate_chunk(self, s, *a, **kw):
            self.calls.append(kw)
            return torch.zeros(len(s.prompts), 3, H, W, dtype=torch.uint8)

    request = dict(context=dict(reference=torch.zeros(1, 3, H, W)), control=dict(control_image=torch.zeros(1, 3, H, W)),
                   true_cfg=dict(negative_prompt="x", true_cfg_scale=4.0), cache=dict(cache_threshold=0.1), controlnet=dict(controlnet_image=torch.zeros(1, 3, H, W)),
                   ip_adapter=dict(ip_adapter_image_embeds=torch.zeros(16)))
    for a, b in PAIRS + MODES:
        pipe = RecordingPipeline()
        pipe.flux.cond_channels = 64 if "control" in (a, b) else 0
        if b == "sequence_parallel":
            pipe._sp = object()
        elif b in ("fp8", "int8"):
            pipe.flux._eight_bit = b
        match = "is not combined with" if (a, b) in PAIRS else ("sequence parallelism" if b == "sequence_parallel" else b + " mode")
        with pytest.raises(ValueError, match=match):
            pipe.generate_tensor(["p"], pl.DiffusionGenerationParams(H, W, 2, 3.5), **request[a], **request.get(b, {}))
        assert not pipe.calls
    # a negative with true_cfg_scale <= 1 is no true CFG: it runs next to the step cache, as ever
    pipe = RecordingPipeline()
    pipe.generate_tensor(["p"], pl.DiffusionGenerationParams(H, W, 2, 3.5), negative_prompt="x", cache_threshold=0.1)
    assert pipe.calls == [{}]
    # each shared option is a keyword of its own, passed only by a request that has it
    pipe.calls.clear()
    pipe.generate_tensor(["p"], pl.DiffusionGenerationParams(H, W, 2, 3.5), **request["controlnet"], **request["ip_adapter"], **request["true_cfg"])
    assert [set(kw) for kw in pipe.calls] == [{"negative", "controlnet", "ip_adapter"}]
    assert isinstance(pipe.calls[0]["controlnet"], pl._ControlNetInput) and isinstance(pipe.calls[0]["ip_adapter"], pl._IpAdapterInput)
