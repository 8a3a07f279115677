"""
The Python binding against include/tmvb.h, without a device (the built library is loaded, nothing is launched):

  * the prototype table of topicmodelsvb.jl_amd/_abi.py names exactly the functions the header declares, and every return and argument type
    is the header's C type under one mapping, position by position;
  * every Structure mirror has the header struct's fields, in order, with the header's types, and every struct a prototype takes has a mirror;
  * nothing outside the table module assigns argtypes / restype;
  * a wrong type stops at the boundary (ctypes.ArgumentError), before the library is entered;
  * the five device models share one base: none redefines the shared methods, none lost or gained a public method.

The header parser lives here, not in the package: the table is the binding, this is its check.
"""
import ctypes as C
import glob
import os
import re
import sys

import pytest

import tmvb_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = tmvb_amd.pkg
ABI = sys.modules[PKG.__name__ + "._abi"]
MODEL = sys.modules[PKG.__name__ + "._model"]

SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint8_t": C.c_uint8, "uint32_t": C.c_uint32, "double": C.c_double,
           "float": C.c_float, "char": C.c_char}


def header():
    text = open(os.path.join(ROOT, "include", "tmvb.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def handles(hdr):
    """the opaque handle types: `typedef struct tmvb_x tmvb_x;`"""
    return set(re.findall(r"typedef\s+struct\s+(tmvb_\w+)\s+\1\s*;", hdr))


def structs(hdr):
    """typedef name -> [(field, C type with its stars)] of every `typedef struct { ... } tmvb_*_t;`"""
    out = {}
    for body, name in re.findall(r"typedef\s+struct\s*\{(.*?)\}\s*(tmvb_\w+_t)\s*;", hdr, flags=re.S):
        fields = []
        for decl in filter(None, (d.strip() for d in body.split(";"))):
            base, rest = re.match(r"([A-Za-z_]\w*)\s*(.*)$", decl, flags=re.S).groups()
            for item in rest.split(","):
                item = item.strip()
                fields.append((item.lstrip("* "), base + "*" * item.count("*")))
        out[name] = fields
    return out


def ctype_of(ctext, hdr_handles, hdr_structs):
    """The mapping of the binding: a C type as the header writes it -> the ctypes type."""
    words = [w for w in re.sub(r"\*", " ", ctext).split() if w != "const"]
    base, stars = words[0], ctext.count("*")
    if base == "tmvb_host_allreduce_fn" and stars == 0:
        return ABI.HOST_ALLREDUCE_FN
    if base == "void":
        return {0: None, 1: C.c_void_p, 2: C.POINTER(C.c_void_p)}[stars]
    if base == "char" and stars == 1:
        return C.c_char_p
    if base in hdr_handles:
        return {1: C.c_void_p, 2: C.POINTER(C.c_void_p)}[stars]
    if base in hdr_structs:
        assert stars == 1, ctext
        assert base in ABI.STRUCTS, f"{base} is passed by pointer but has no Structure mirror"
        return C.POINTER(ABI.STRUCTS[base])
    return {0: SCALARS[base], 1: C.POINTER(SCALARS[base])}[stars]


def prototypes(hdr):
    found = re.findall(r"\b([A-Za-z_][\w \*]*?)\b(tmvb_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", hdr)
    out = {}
    for ret, name, args in found:
        args = " ".join(args.split())
        params = [] if args in ("", "void") else [re.sub(r"\b\w+$", "", a.strip()) if not a.strip().endswith("*") else a.strip() for a in args.split(",")]
        out[name] = (ret.strip(), params)
    return out


def test_table_matches_the_header(tmvb):
    hdr = header()
    H, S, P = handles(hdr), structs(hdr), prototypes(hdr)
    assert len(P) > 100
    assert sorted(ABI.PROTOTYPES) == tmvb.exported_symbols() == sorted(P)
    assert list(ABI.PROTOTYPES) == list(P), "the table keeps the header's order"
    for name, (ret, params) in P.items():
        restype, argtypes = ABI.PROTOTYPES[name]
        assert restype is ctype_of(ret, H, S), (name, ret, restype)
        assert len(argtypes) == len(params), (name, params, argtypes)
        for q, (ctext, at) in enumerate(zip(params, argtypes)):
            assert at is ctype_of(ctext, H, S), (name, q, ctext, at)
    assert ABI.PROTOTYPES["tmvb_last_error"][0] is C.c_char_p
    for name in ("tmvb_docfile_free", "tmvb_gencorp_free", "tmvb_split_free", "tmvb_rsplit_free"):
        assert ABI.PROTOTYPES[name][0] is None
    L = tmvb.lib()                                   # and lib() has applied it
    for name, (restype, argtypes) in ABI.PROTOTYPES.items():
        fn = getattr(L, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name


def test_struct_mirrors_match_the_header():
    hdr = header()
    H, S = handles(hdr), structs(hdr)
    assert len(S) > 10
    assert set(ABI.STRUCTS) <= set(S), "a mirror of a struct the header does not have"
    by_pointer = {w for _, params in prototypes(hdr).values() for p in params for w in p.replace("*", " ").split() if w in S}
    assert by_pointer <= set(ABI.STRUCTS), f"passed by pointer without a mirror: {sorted(by_pointer - set(ABI.STRUCTS))}"
    for name, cls in ABI.STRUCTS.items():
        assert issubclass(cls, C.Structure)
        want = [(f, ctype_of(t, H, S)) for f, t in S[name]]
        assert [(f, t) for f, t in cls._fields_] == want, name
    # the names the package had before the table still resolve, and to these classes
    for mod, names in (("_lib", ("CorpusInfo", "RecTopNInfo", "SearchInfo", "TokenTopicsInfo", "FoldinInfo")), ("heldout", ("SplitResult",)),
                       ("gencorp", ("GenCorpResult",)), ("recs_eval", ("ReaderSplit", "RecRanksInfo")), ("neighbors", ("NeighborsInfo",)),
                       ("coherence", ("CodfInfo",)), ("lda_svi", ("SviInfo",)), ("ctm_svi", ("SviInfo",)), ("cluster", ("KMeansInfo",)),
                       ("docmap", ("MapParams", "MapInfo"))):
        m = sys.modules[PKG.__name__ + "." + mod]
        for n in names:
            assert getattr(m, n) is getattr(ABI, n), (mod, n)
    lib_mod = sys.modules[PKG.__name__ + "._lib"]
    for n, t in (("P_i64", C.c_int64), ("P_i32", C.c_int32), ("P_dbl", C.c_double), ("P_f32", C.c_float)):
        assert getattr(lib_mod, n) is C.POINTER(t)
    assert lib_mod.VP is C.c_void_p


def test_no_prototype_outside_the_table():
    files = sorted(glob.glob(os.path.join(ROOT, "topicmodelsvb.jl_amd", "**", "*.py"), recursive=True))
    assert len(files) > 20
    for f in files:
        if os.path.basename(f) == "_abi.py":
            continue
        for k, line in enumerate(open(f), start=1):
            assert not re.search(r"\.(argtypes|restype)\b[^=\n]*=(?!=)", line), f"{f}:{k}: {line.strip()}"


def test_wrong_types_stop_at_the_boundary(tmvb):
    L = tmvb.lib()
    with pytest.raises(C.ArgumentError):
        L.tmvb_digamma_f64(None, None, 2.5)                   # a float for an int64_t
    with pytest.raises(C.ArgumentError):
        L.tmvb_lda_estep(None, C.c_int64(1), 0.0)             # an int64 wrapper for an int32_t
    with pytest.raises(C.ArgumentError):
        L.tmvb_lda_set_distributed(None, C.c_int32(1), 0)     # and an int32 wrapper for an int64_t


SHARED = ("close", "__del__", "update_elbo", "elbo_form", "doc_sweeps", "synchronize")
PUBLIC = {      # the public methods of the classes as they were before they shared a base
    "gpuLDA": "bind_stats close doc_sweeps elbo_form estep estep_allreduce estep_launches estep_pieces last_estep_ms reduce_docs set_comm set_distributed "
              "stats sweep_hist synchronize train update_alpha update_beta update_buffer update_elbo update_host",
    "gpufLDA": "close doc_sweeps elbo_form estep last_estep_ms mstep reduce_docs set_comm synchronize train update_alpha update_beta update_buffer "
               "update_elbo update_eta update_host",
    "gpuCTM": "bind_stats close doc_sweeps elbo_form estep last_estep_ms reduce_docs set_comm set_distributed solver_stats stats sweep_hist synchronize "
              "train update_beta update_buffer update_elbo update_host update_mu update_sigma",
    "gpufCTM": "close doc_sweeps elbo_form estep mstep reduce_docs set_comm sweep_hist synchronize train update_beta update_buffer update_elbo "
               "update_host update_mu update_sigma",
    "gpuCTPF": "bind_stats close doc_sweeps elbo_form estep hyper last_estep_ms mstep recommend recommend_topn reduce_docs set_comm set_distributed "
               "stats sweep_hist synchronize train update_buffer update_elbo update_elbo_parts update_host",
}


@pytest.mark.parametrize("name", sorted(PUBLIC))
def test_models_share_the_base(tmvb, name):
    cls = getattr(tmvb, name)
    assert issubclass(cls, MODEL.DeviceModel)
    for m in SHARED:
        assert m not in cls.__dict__, f"{name} redefines {m}"
        assert getattr(cls, m) is getattr(MODEL.DeviceModel, m)
    public = sorted(n for n in dir(cls) if not n.startswith("_") and callable(getattr(cls, n)))
    assert public == PUBLIC[name].split()
    prefix = f"tmvb_{cls._ABI}_"                           # and no method without its ABI function (tmvb_fctm_stats does not exist)
    for n in ("stats", "bind_stats", "last_estep_ms", "set_distributed", "update_alpha", "update_sigma", "update_eta", "solver_stats", "estep_allreduce"):
        if n in public:
            assert prefix + n in ABI.PROTOTYPES, (name, n)
