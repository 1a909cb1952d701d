"""ctypes view of the internal stencil launchers of ``csrc/stencil.hip`` and of ``bk_problem::jvp_axpy_dot`` (``csrc/problem.hip``),
for the kernel tests -- the pattern of ``tests/vecops_abi.py``.

The Makefile hides no symbols, so ``libbkhip.so`` exports the launchers under their Itanium-mangled names.  A mangled name encodes
the NAME of an argument struct, not its layout: ``test_stencil_coverage_host.py`` therefore parses the three struct bodies out of
``csrc/ops.h`` and compares field names, order, C types and default member values with the mirrors below.  ``include/bkhip.h`` stays
the public ABI; these names are a test-only view of the same library.
"""
import ctypes as C

P, Z, I, D = C.c_void_p, C.c_size_t, C.c_int, C.c_double

# C type as written in ops.h -> ctypes type (device pointers travel as raw addresses)
CTYPES = {"int": C.c_int, "double": C.c_double, "bool": C.c_bool, "const double*": C.c_void_p, "double*": C.c_void_p,
          "int*": C.POINTER(C.c_int)}

# (field, C type, default member value or None) in declaration order
SH_ARGS = [("nx", "int", None), ("ny", "int", None), ("nz", "int", None), ("nzg", "int", None), ("zoff", "int", None),
           ("ax", "double", None), ("ay", "double", None), ("az", "double", None), ("l", "double", None), ("nu", "double", None),
           ("a0", "double", None), ("a1", "double", None), ("ag", "double", 0.0), ("ag_set", "bool", False), ("mode", "int", None),
           ("v", "const double*", None), ("u", "const double*", None), ("out", "double*", None),
           ("halo_lo", "const double*", None), ("halo_hi", "const double*", None), ("part", "int", 0),
           ("dot_blocks", "int*", None), ("addv", "const double*", None), ("addc", "double", 0.0)]
CGL_ARGS = [("nx", "int", None), ("ny", "int", None), ("ax", "double", None), ("ay", "double", None), ("r", "double", None),
            ("mu", "double", None), ("nu", "double", None), ("c3", "double", None), ("c5", "double", None), ("gamma", "double", None),
            ("a0", "double", None), ("a1", "double", None), ("mode", "int", None), ("v", "const double*", None),
            ("u", "const double*", None), ("out", "double*", None)]
SH1D_ARGS = [("nx", "int", None), ("ax", "double", None), ("lam", "double", None), ("nu", "double", None), ("a0", "double", None),
             ("a1", "double", None), ("mode", "int", None), ("v", "const double*", None), ("u", "const double*", None),
             ("out", "double*", None)]
# members whose C++ default is a null pointer (`= nullptr`): ctypes zero-initialises, spelled out in the constructors below
NULL_DEFAULTS = {"ShArgs": ("dot_blocks", "addv")}


def _mirror(name, table):
    defaults = {f: d for f, _, d in table if d is not None}

    def __init__(self, **kw):
        C.Structure.__init__(self)
        for f, d in defaults.items():            # the default member values of the C++ struct, explicitly
            setattr(self, f, d)
        for f in NULL_DEFAULTS.get(name, ()):
            setattr(self, f, None)
        for f, v in kw.items():
            if f not in self._names:
                raise TypeError(f"{name} has no field {f}")
            setattr(self, f, v)
    return type(name, (C.Structure,), {"_fields_": [(f, CTYPES[t]) for f, t, _ in table], "_names": {f for f, _, _ in table},
                                       "__init__": __init__})


ShArgs = _mirror("ShArgs", SH_ARGS)
CglArgs = _mirror("CglArgs", CGL_ARGS)
Sh1dArgs = _mirror("Sh1dArgs", SH1D_ARGS)
STRUCTS = {"ShArgs": SH_ARGS, "CglArgs": CGL_ARGS, "Sh1dArgs": SH1D_ARGS}

# mangled name -> (short name, argtypes, restype).  The argument structs go by const reference (= a pointer); the first argument of
# the member function jvp_axpy_dot is the bk_problem* handle; params, dot and fused are host memory
LAUNCHERS = {
    "_ZN2bk8sh_applyEP6bk_ctxRKNS_6ShArgsE": ("sh_apply", [P, C.POINTER(ShArgs)], I),
    "_ZN2bk15sh_fused_dot_okEP6bk_ctxRKNS_6ShArgsE": ("sh_fused_dot_ok", [P, C.POINTER(ShArgs)], C.c_bool),
    "_ZN2bk9cgl_applyEP6bk_ctxRKNS_7CglArgsE": ("cgl_apply", [P, C.POINTER(CglArgs)], I),
    "_ZN2bk10sh1d_applyEP6bk_ctxRKNS_8Sh1dArgsE": ("sh1d_apply", [P, C.POINTER(Sh1dArgs)], I),
    "_ZN2bk10pde_dparamEP6bk_ctxiimdPKdPd": ("pde_dparam", [P, I, I, Z, D, P, P], I),
    "_ZN10bk_problem12jvp_axpy_dotEPKdS1_S1_dddS1_PdS2_Pi":
        ("jvp_axpy_dot", [P, P, P, C.POINTER(C.c_double), D, D, D, P, P, C.POINTER(C.c_double), C.POINTER(C.c_int)], I),
}

# constants of csrc/stencil.hip and csrc/common.h the tests' shapes depend on
TX, TY = 64, 16                  # tile of sh_stream_kernel
NT_POINTS = 1 << 22              # sh_nt: non-temporal loads / stores from this many points on
DPARAM_GRID_CAP = 4096           # dparam_kernel: blocks of 256 threads, grid-stride beyond
K_PARTIAL_DOUBLES = 1024 * 72    # kPartialDoubles: most tiles the fused dot can have


class Launchers:
    """Attribute access to the launchers of one loaded library: ``Launchers(lib).sh_apply(ctx.h, byref(args))``."""

    def __init__(self, lib):
        for mangled, (name, argtypes, restype) in LAUNCHERS.items():
            f = getattr(lib, mangled)            # AttributeError: the symbol (= that signature) is gone
            f.argtypes, f.restype = argtypes, restype
            setattr(self, name, f)
