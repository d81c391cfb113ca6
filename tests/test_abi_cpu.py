"""The ctypes binding and the enum values are derived from include/henbun_hip.h (henbun_amd/_lib.py).  No GPU needed:
a C++ compiler confirms that the parser reads the header the way the compiler does, the parser's edge cases are
exercised on hand-written text, every `call("hb_...")` site of the package is held to its prototype's argument count,
and hip_ops' constants and the INTEGRATION.md stub are compared with what the header says."""
import ast
import ctypes
import glob
import os
import re
import shutil
import subprocess
from ctypes import c_char_p, c_double, c_int, c_long, c_uint64, c_void_p

import pytest

from henbun_amd import _build, _lib, hip_ops as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CLASS = {c_void_p: "P", c_int: "I", c_long: "L", c_double: "D", c_uint64: "U", c_char_p: "S"}


def _signatures():
    with open(os.path.join(ROOT, "include", "henbun_hip.h")) as f:
        return _lib.parse_prototypes(f.read())


def _classes(restype, argtypes):
    return "".join(_CLASS[t] for t in [restype] + list(argtypes))


# ---------------------------------------------------------------- a. the compiler is the parser's oracle
_SIG_CHECK = r"""
#include <cstdint>
#include <type_traits>
#include "henbun_hip.h"
template <class T> constexpr char cls() {
  return std::is_same<T, const char*>::value ? 'S' : std::is_pointer<T>::value ? 'P'
       : std::is_same<T, int>::value ? 'I' : std::is_same<T, long>::value ? 'L' : std::is_same<T, double>::value ? 'D'
       : (std::is_same<T, uint64_t>::value || std::is_same<T, unsigned long long>::value) ? 'U' : '?';
}
template <class R, class... A> constexpr bool sig(R (*)(A...), const char* want) {
  /* the return keeps `const char*` apart ('S'); among the parameters every pointer is 'P' */
  const char got[] = {cls<R>(), (std::is_pointer<A>::value ? 'P' : cls<A>())..., 0};
  for (int i = 0;; ++i) {
    if (got[i] != want[i]) return false;
    if (!got[i]) return true;
  }
}
"""


def _host_cxx():
    for cand in ("c++", "g++"):
        if shutil.which(cand):
            return shutil.which(cand)
    clang = os.path.join(os.path.dirname(os.path.realpath(_build._hipcc())), "..", "lib", "llvm", "bin", "clang++")
    assert os.path.exists(clang), "no host C++ compiler: neither c++ nor g++ on PATH, nor hipcc's clang++ at " + clang
    return clang


def _syntax_check(source, tmp_path):
    src = tmp_path / "abi_check.cpp"
    src.write_text(source)
    return subprocess.run([_host_cxx(), "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                          capture_output=True, text=True)


def _assertions(sigs, consts):
    lines = ['static_assert(sig(&%s, "%s"), "%s");' % (n, _classes(*s), n) for n, s in sigs.items()]
    lines += ['static_assert(%s == %d, "%s");' % (n, v, n) for n, v in consts.items()]
    return "\n".join(lines) + "\n"


def test_compiler_agrees_with_every_parsed_signature_and_constant(tmp_path):
    sigs, consts = _signatures(), _lib.constants()
    assert len(sigs) >= 192 and len(consts) >= 90   # with hb_matmul_form and HB_MM_FORM_* (profiles/abi_binding.txt, 5)
    assert "hb_matmul_form" in sigs and consts["HB_MM_FORM_ROWSREG"] == 4
    r = _syntax_check(_SIG_CHECK + _assertions(sigs, consts), tmp_path)
    assert r.returncode == 0, r.stderr[-4000:]
    # the same oracle for the forms the real header does not use today (an enum whose first value is implicit, ...)
    edge = _SIG_CHECK.replace('#include "henbun_hip.h"', _EDGE_HEADER)
    r = _syntax_check(edge + _assertions(_lib.parse_prototypes(_EDGE_HEADER), _lib.parse_constants(_EDGE_HEADER)), tmp_path)
    assert r.returncode == 0, r.stderr[-4000:]
    # the check has teeth: one wrong class, and one wrong value, fail with the entry's name in the message
    bad = _classes(*sigs["hb_fill_f32"]).replace("L", "I")
    r = _syntax_check(_SIG_CHECK + 'static_assert(sig(&hb_fill_f32, "%s"), "hb_fill_f32");\n' % bad, tmp_path)
    assert r.returncode != 0 and "hb_fill_f32" in r.stderr
    r = _syntax_check(_SIG_CHECK + 'static_assert(HB_EW_EXP == 1, "HB_EW_EXP");\n', tmp_path)
    assert r.returncode != 0 and "HB_EW_EXP" in r.stderr


# ---------------------------------------------------------------- b. parser edge cases
_EDGE_HEADER = """
/* a comment with int hb_not_a_function(void); inside */
#ifndef X
#define HB_SOME_BYTES 0x80
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
enum { HB_A = 3, HB_B, HB_C = HB_A | 8, HB_D, HB_NEG = -2, HB_E, };
enum { HB_Z /* implicit first value */, HB_Y };
int hb_ptrs(const void* const* in, void** handle_out, char* buf, const char* key);  // trailing comment
int hb_u64(unsigned long long* out, uint64_t seed, unsigned long long n);
int hb_three_lines(int a, /* comment, with (parens); */ long b,
                   double c,
                   const float *d);
int hb_nothing(void);
int hb_empty();
long hb_count(long n);
const char* hb_name(void);
const char *hb_name2(void);
#ifdef __cplusplus
}
#endif
#endif
"""


def test_parser_reads_the_forms_the_header_uses():
    sigs = _lib.parse_prototypes(_EDGE_HEADER)
    assert list(sigs) == ["hb_ptrs", "hb_u64", "hb_three_lines", "hb_nothing", "hb_empty", "hb_count", "hb_name", "hb_name2"]
    assert sigs["hb_ptrs"] == (c_int, [c_void_p] * 4)
    assert sigs["hb_u64"] == (c_int, [c_void_p, c_uint64, c_uint64])
    assert sigs["hb_three_lines"] == (c_int, [c_int, c_long, c_double, c_void_p])
    assert sigs["hb_nothing"] == (c_int, []) and sigs["hb_empty"] == (c_int, [])
    assert sigs["hb_count"] == (c_long, [c_long])
    assert sigs["hb_name"] == (c_char_p, []) and sigs["hb_name2"] == (c_char_p, [])


@pytest.mark.parametrize("decl", [
    "int hb_bad(float x);", "int hb_bad(long n, size_t m);", "float hb_bad(long n);", "void* hb_bad(void);",
    "int hb_bad(unsigned long long);", "int hb_bad(long long n);", "int hb_bad(long n)", "struct hb_bad { int x; };",
])
def test_parser_never_guesses_a_type(decl):
    with pytest.raises(ValueError, match="hb_bad"):
        _lib.parse_prototypes("int hb_ok(void);\n" + decl + "\nint hb_ok2(void);\n")


def test_constants_follow_the_rules_of_c_enums():
    c = _lib.parse_constants(_EDGE_HEADER)
    assert c == dict(HB_SOME_BYTES=128, HB_A=3, HB_B=4, HB_C=11, HB_D=12, HB_NEG=-2, HB_E=-1, HB_Z=0, HB_Y=1)
    with pytest.raises(ValueError, match="HB_Q"):
        _lib.parse_constants("enum { HB_Q = sizeof(int) };")
    real = _lib.constants()
    assert real["HB_ABI_VERSION"] == 2 and real["HB_COMM_ID_BYTES"] == 128 and real["HB_EW_DIGAMMA"] == 22


def test_declared_symbols_are_the_parsed_names():
    assert _lib.declared_symbols() == list(_signatures())
    lib = _lib.lib()
    for name, (restype, argtypes) in _signatures().items():
        fn = lib.raw(name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name


# ---------------------------------------------------------------- c. every call site passes its prototype's count
# sites whose entry name is computed (a deferred side job or its stand-alone twin): not checked statically
_COMPUTED_NAME_SITES = {"launch_draw", "diag_sample_kl_fwd", "diag_sample_kl_bwd"}


class _CallSites(ast.NodeVisitor):
    """(line, enclosing function, [entry names] or None for a computed name, argument count or None when starred) of
    every `<expr>.call("hb_...", ...)`, `<expr>.call("hb_..." + <suffix>, ...)` and `<expr>.call(<other expression>, ...)`."""

    def __init__(self):
        self.scope, self.found = ["<module>"], []

    def visit_FunctionDef(self, node):
        self.scope.append(node.name)
        self.generic_visit(node)
        self.scope.pop()

    def visit_Call(self, node):
        self.generic_visit(node)
        if not (isinstance(node.func, ast.Attribute) and node.func.attr == "call" and node.args):
            return
        first = node.args[0]
        if isinstance(first, ast.Constant) and isinstance(first.value, str):
            names = [first.value]
        elif isinstance(first, ast.BinOp) and isinstance(first.op, ast.Add) and isinstance(first.left, ast.Constant):
            names = [str(first.left.value) + "_f32", str(first.left.value) + "_f64"]   # the typed pair
        else:
            names = None
        if names and not names[0].startswith("hb_"):
            return   # some other object's .call
        starred = any(isinstance(a, ast.Starred) for a in node.args) or bool(node.keywords)
        self.found.append((node.lineno, self.scope[-1], names, None if starred else len(node.args) - 1))


def _call_sites():
    out = []
    for path in sorted(glob.glob(os.path.join(ROOT, "henbun_amd", "**", "*.py"), recursive=True)):
        visitor = _CallSites()
        with open(path) as f:
            visitor.visit(ast.parse(f.read()))
        out += [(os.path.relpath(path, ROOT),) + site for site in visitor.found]
    return out


def test_every_call_site_passes_exactly_the_declared_arguments():
    sigs = _signatures()
    sites = _call_sites()
    skipped = [s for s in sites if s[3] is None]
    assert {s[2] for s in skipped} == _COMPUTED_NAME_SITES and len(skipped) == 3, skipped
    pairs, failures = 0, []
    for path, line, _, names, nargs in sites:
        for name in names or []:
            pairs += 1
            if name not in sigs:
                failures.append("%s:%d: %s is not declared" % (path, line, name))
            elif nargs is None:
                failures.append("%s:%d: %s is called with starred or keyword arguments" % (path, line, name))
            elif nargs != len(sigs[name][1]):
                failures.append("%s:%d: %s takes %d arguments, %d given" % (path, line, name, len(sigs[name][1]), nargs))
    assert not failures, "\n".join(failures)
    assert pairs > 100, pairs   # the walk did find the package's call sites (133 pairs when this test was written)


# ---------------------------------------------------------------- d. call() holds the count at run time
def test_call_rejects_a_wrong_argument_count_before_entering_the_library():
    lib = _lib.lib()
    lib.call("hb_debug_clear")
    with pytest.raises(TypeError, match=r"hb_debug_clear takes 0 arguments \(1 given\)"):
        lib.call("hb_debug_clear", 0)
    with pytest.raises(TypeError, match=r"hb_debug_set takes 2 arguments \(1 given\)"):
        lib.call("hb_debug_set", b"chol_persist")
    lib.call("hb_debug_set", b"chol_persist", 1)   # bytes bind to the `const char*` parameter
    lib.call("hb_debug_clear")


# ---------------------------------------------------------------- e. hip_ops' constants are the header's
def test_hip_ops_constants_are_the_headers():
    c = _lib.constants()
    assert H.EW == {k[len("HB_EW_"):]: v for k, v in c.items() if k.startswith("HB_EW_") and k != "HB_EW_PROG_SUM"}
    assert len(H.EW) == 43 and "PROG_SUM" not in H.EW
    assert H.ACT == {"none": c["HB_ACT_NONE"], "sigmoid": c["HB_ACT_SIGMOID"], "relu": c["HB_ACT_RELU"],
                     "tanh": c["HB_ACT_TANH"]}
    required = ("EW_PROG_SUM RED_SUM RED_MAX KERN_RBF KERN_CSYM_RBF KERN_SQDIST KERN_KBAR_SYMMETRIC MM_LOWER_OUT "
                "MM_TRIL_OUT MM_PHI_OUT MM_SYM_OUT MM_SYMLOW_OUT MM_ACTGRAD SGP_NEGLECTED SGP_DIAGONAL SGP_FULLRANK "
                "SGP_S_DIAG SGP_S_TRIL PREC_NATIVE PREC_BF16X3 LIK_GAUSSIAN LIK_BERNOULLI LIK_POISSON COLPROG_SUM "
                "COLPROG_MAX").split()
    for name in required:
        assert getattr(H, name) == c["HB_" + name], name
    # and no other public constant of hip_ops shadows a header name with another value
    for name, value in vars(H).items():
        if name.isupper() and "HB_" + name in c:
            assert value == c["HB_" + name], name


# ---------------------------------------------------------------- f. the stub of INTEGRATION.md binds the same types
def test_integration_stub_binds_the_derived_signatures(monkeypatch):
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    section = text[text.index("## 1."):text.index("## 2.")]
    block = re.search(r"```python\n(.*?)```", section, re.S).group(1)
    handle = ctypes.CDLL(_lib.LIB_PATH)   # its own handle: the stub's argtypes do not touch the package's binding
    monkeypatch.setattr(ctypes, "CDLL", lambda *a, **k: handle)
    exec(compile(block, "INTEGRATION.md", "exec"), {"__file__": os.path.join(ROOT, "Henbun", "hip_backend.py")})
    sigs = _signatures()

    def cls(t):
        pointer = issubclass(t, (c_void_p, c_char_p, ctypes._Pointer))
        return "P" if pointer else _CLASS[t]

    bound = [n for n, fn in vars(handle).items() if n.startswith("hb_") and fn.argtypes is not None]
    assert len(bound) >= 8, bound
    for name in bound:
        want = "".join("P" if t is c_void_p else _CLASS[t] for t in sigs[name][1])
        assert "".join(cls(t) for t in getattr(handle, name).argtypes) == want, name
