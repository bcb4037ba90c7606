"""CPU: the C ABI keeps its promise that nothing unwinds across it (include/bpp_amd.h, Conventions).

 * csrc/abi_guard.hpp built for the host (g++, under the sanitizers with BPP_HOST_SANITIZE=1): each kind of exception
   becomes its return code and text, a normal return passes through, a count of 2^32 or more is rejected.
 * capi.hip: every extern "C" definition routes its body through the guard or a guarded shim, except the few that cannot
   throw, and none sets the device by hand.  It stages no buffer: the host forms do, through csrc/staging.hpp alone.
 * the ctypes binding (_lib.py) states every prototype of the header: arity, pointer or scalar, scalar width, return."""

import ctypes
import os
import re
import subprocess
import sys

from test_host_arith_cpu import _build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_rust_ffi as G  # noqa: E402

# extern "C" definitions that need no guard
UNGUARDED = {
    "bpp_last_error": "returns the stored text",
    "bpp_point_words": "a switch on the curve id",
    "bpp_point_compressed_bytes": "a switch on the curve id",
    "bpp_point_uncompressed_bytes": "a switch on the curve id",
    "bpp_proof_bytes": "arithmetic on its arguments",
    "bpp_proof_bytes_version": "arithmetic on its arguments",
    "bpp_verifier_msm_len": "reads a field",
    "bpp_verifier_table_bytes": "reads a field",
    "bpp_verifier_dominant_kernel": "returns a literal",
    "bpp_verifier_set_subgroup_check": "sets a field",
    "bpp_destroy": "destructors only (hipFree, hipEventDestroy), which do not throw",
    "bpp_verifier_destroy": "destructors only",
    "bpp_graph_destroy": "destructors only",
    "bpp_proofs_encode": "forwards to bpp_proofs_encode_version",
}
SHIMS = ("guarded(", "on_ctx(", "on_device(", "size_for(")


def test_guard_maps_exceptions_to_codes(tmp_path):
    out = subprocess.run([_build("abi_guard_host_test", tmp_path)], capture_output=True, text=True)
    assert out.returncode == 0 and "ok abi_guard" in out.stdout, out.stdout + out.stderr


def _entry_points(src):
    """-> {name: (text before the body, body)} of every extern "C" definition in capi.hip"""
    src = re.sub(r"//[^\n]*", "", src)
    out = {}
    for m in re.finditer(r'extern "C"[^;{]*?\b(bpp_\w+)\s*\(', src):
        i = src.index("{", m.end())
        if ";" in src[m.end():i]:
            continue   # a declaration
        depth, j = 0, i
        while True:
            depth += {"{": 1, "}": -1}.get(src[j], 0)
            if depth == 0:
                break
            j += 1
        out[m.group(1)] = src[i + 1:j]
    return out


def test_every_entry_point_runs_under_the_guard():
    entries = _entry_points(open(os.path.join(ROOT, "bulletproofsplus_amd", "csrc", "capi.hip")).read())
    assert len(entries) >= 70 and set(UNGUARDED) <= set(entries), set(UNGUARDED) - set(entries)
    for name, body in entries.items():
        assert "hipSetDevice" not in body, (name, "sets the device by hand instead of through on_device / on_ctx")
        if name in UNGUARDED:
            continue
        at = [body.find(s) for s in SHIMS if s in body]
        assert at, (name, "runs outside guarded / on_ctx / on_device / size_for")
        # before the shim only argument checks: nothing that can allocate, throw or reach the device
        head = body[:min(at)]
        assert not re.search(r"\bhip\w*\(|\bnew\b|std::|DevBuf|HIPCHK|\bImpl\b|Impl<", head), (name, head)


CSRC = os.path.join(ROOT, "bulletproofsplus_amd", "csrc")


def _receiver_check(name):
    """-> the body of scan_args or find_args, the one check in front of the receiver's entries (csrc/scan_args.hpp)"""
    text = open(os.path.join(CSRC, "scan_args.hpp")).read()
    at = text.index("inline int %s(" % name)
    return text[at:text.index("\n}\n", at)]


def _csrc_sources():
    """-> {file name: text} of the library's sources"""
    return {f: open(os.path.join(CSRC, f)).read() for f in sorted(os.listdir(CSRC)) if f.endswith((".hip", ".hpp", ".h"))}


def test_host_forms_stage_through_one_vocabulary():
    src = _csrc_sources()
    assert len(src) > 40 and "capi.hip" in src and "staging.hpp" in src
    # capi.hip is the boundary: argument checks and shims, no buffer of its own
    named = re.findall(r"DevBuf|hipMemcpy|hipMalloc|hipMemset", src["capi.hip"])
    assert not named, ("capi.hip names", sorted(set(named)))
    # one allocation site: DevBuf::alloc
    sites = [(f, m.start()) for f, text in src.items() for m in re.finditer(r"hipMalloc\(", text)]
    assert [f for f, _ in sites] == ["staging.hpp"], sites
    text = src["staging.hpp"]
    a = text.index("hipError_t alloc(size_t n) {")
    assert a < sites[0][1] < text.index("}", a), "hipMalloc( outside DevBuf::alloc"
    # no copy whose return code is thrown away
    ignored = [(f, m.group(0)) for f, text in src.items() for m in re.finditer(r"\(void\)\s*hipMemcpy\w*", text)]
    assert not ignored, ignored
    # the debug kernels live in tu_debug.hip, not in the units of the hot MSM kernels
    assert "k_dbg_" not in src["impl_msm.hpp"] and "k_dbg_field<" in src["tu_debug.hip"] and "k_dbg_point<" in src["tu_debug.hip"]
    # the six copies of the staging rule are gone
    for name in ("verify_staged", "prove_mixed_staged", "upload_optional", "KeyUpload", "wip_upload"):
        assert not any(re.search(r"\b%s\b" % name, text) for text in src.values()), name
    assert not re.search(r"\bint upload\(DevBuf", src["tu_debug.hip"])


def _width(ct):
    """(bytes, signed) of a ctypes scalar type"""
    return ctypes.sizeof(ct), ct(-1).value < 0


C_SCALAR = {"int": (4, True), "unsigned": (4, False), "uint32_t": (4, False), "size_t": (8, False), "uint64_t": (8, False)}


def _is_pointer(ct):
    return ct in (ctypes.c_void_p, ctypes.c_char_p) or issubclass(ct, ctypes._Pointer)


def test_python_binding_matches_the_header():
    from bulletproofsplus_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    L = _lib.lib()
    protos = G.c_prototypes(open(os.path.join(ROOT, "include", "bpp_amd.h")).read())
    assert {n for n, _, _ in protos} == set(_lib.EXPORTS)
    for name, (rb, rc, rs), ps in protos:
        f = getattr(L, name)
        args = f.argtypes or []
        assert len(args) == len(ps), (name, "arity", len(args), len(ps))
        for (pn, b, c, s), ct in zip(ps, args):
            if s:
                assert _is_pointer(ct), (name, pn, "a pointer in the header", ct)
            else:
                assert not _is_pointer(ct) and _width(ct) == C_SCALAR[b], (name, pn, b, ct)
        if rs:
            assert (rb, rs) == ("char", 1) and f.restype is ctypes.c_char_p, (name, "return", f.restype)
        elif rb == "void":
            assert f.restype is None, (name, "void return", f.restype)
        else:
            assert f.restype is not None and not _is_pointer(f.restype) and _width(f.restype) == C_SCALAR[rb], \
                (name, "return", rb, f.restype)
