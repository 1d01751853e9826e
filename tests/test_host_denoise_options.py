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
