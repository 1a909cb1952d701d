"""ctypes table of the internal ``bk::v_*`` launchers of ``csrc/vecops.hip``, for the kernel tests.

The Makefile does not hide symbols, so ``libbkhip.so`` exports every launcher under its Itanium-mangled C++ name.  The
mangled name encodes the parameter list: a launcher whose signature changes no longer resolves, and the lookup fails loudly
instead of calling it with the wrong arguments.  ``include/bkhip.h`` stays the public ABI (``test_capi_symbols.py``); these
names are a test-only view of the same library.
"""
import ctypes as C

P, Z, I, D, U64 = C.c_void_p, C.c_size_t, C.c_int, C.c_double, C.c_ulonglong

# mangled name -> (short name, argtypes, restype).  Pointers are raw addresses: device memory (torch tensors) for vectors, host
# memory (numpy arrays) for outputs and coefficient tables, as the launcher's contract says.
LAUNCHERS = {
    "_ZN2bk6v_copyEP6bk_ctxmPKdPd": ("v_copy", [P, Z, P, P], I),
    "_ZN2bk6v_zeroEP6bk_ctxmPd": ("v_zero", [P, Z, P], I),
    "_ZN2bk8v_axpbyzEP6bk_ctxmdPKddS3_Pd": ("v_axpbyz", [P, Z, D, P, D, P, P], I),
    "_ZN2bk7v_axpbyEP6bk_ctxmdPKddPd": ("v_axpby", [P, Z, D, P, D, P], I),
    "_ZN2bk7v_scaleEP6bk_ctxmdPd": ("v_scale", [P, Z, D, P], I),
    "_ZN2bk10v_pw_scaleEP6bk_ctxmPKdS3_dddPd": ("v_pw_scale", [P, Z, P, P, D, D, D, P], I),
    "_ZN2bk13v_fill_randomEP6bk_ctxmmyPd": ("v_fill_random", [P, Z, Z, U64, P], I),
    "_ZN2bk5v_dotEP6bk_ctxmPKdS3_Pd": ("v_dot", [P, Z, P, P, P], I),
    "_ZN2bk6v_dot2EP6bk_ctxmPKdS3_S3_Pd": ("v_dot2", [P, Z, P, P, P, P], I),
    "_ZN2bk6v_nrm2EP6bk_ctxmPKdPd": ("v_nrm2", [P, Z, P, P], I),
    "_ZN2bk8v_nrminfEP6bk_ctxmPKdPd": ("v_nrminf", [P, Z, P, P], I),
    "_ZN2bk11v_diff_nrm2EP6bk_ctxmPKdS3_Pd": ("v_diff_nrm2", [P, Z, P, P, P], I),
    "_ZN2bk10v_axpy_dotEP6bk_ctxmdPKdPdS3_S4_": ("v_axpy_dot", [P, Z, D, P, P, P, P], I),
    "_ZN2bk15v_minres_updateEP6bk_ctxmdPKddS3_dS3_PddS4_": ("v_minres_update", [P, Z, D, P, D, P, D, P, P, D, P], I),
    "_ZN2bk16v_minres_update2EP6bk_ctxmdPKddddS3_ddS3_S3_PdS4_ddS4_":
        ("v_minres_update2", [P, Z, D, P, D, D, D, P, D, D, P, P, P, P, D, D, P], I),
    "_ZN2bk10v_multidotEP6bk_ctxmPKdmiS3_Pd": ("v_multidot", [P, Z, P, Z, I, P, P], I),
    "_ZN2bk18v_multidot_gram_okEP6bk_ctxmPKdmiS3_": ("v_multidot_gram_ok", [P, Z, P, Z, I, P], C.c_bool),
    "_ZN2bk15v_multidot_gramEP6bk_ctxmPKdmiS3_PdS4_": ("v_multidot_gram", [P, Z, P, Z, I, P, P, P], I),
    "_ZN2bk11v_multiaxpyEP6bk_ctxmPKdmiS3_S3_dPdS4_": ("v_multiaxpy", [P, Z, P, Z, I, P, P, D, P, P], I),
    "_ZN2bk10v_block_okEP6bk_ctxmPKdm": ("v_block_ok", [P, Z, P, Z], C.c_bool),
    "_ZN2bk12v_block_dotsEP6bk_ctxmPKdmiiiPdS4_": ("v_block_dots", [P, Z, P, Z, I, I, I, P, P], I),
    "_ZN2bk12v_block_axpyEP6bk_ctxmPdmiiPKdS4_": ("v_block_axpy", [P, Z, P, Z, I, I, P, P], I),
    "_ZN2bk18v_arnoldi_step_devEP6bk_ctxmPdmiPKdddS2_S2_S2_": ("v_arnoldi_step_dev", [P, Z, P, Z, I, P, D, D, P, P, P], I),
    "_ZN2bk15v_basis_combineEP6bk_ctxmPKdmiS3_iPdm": ("v_basis_combine", [P, Z, P, Z, I, P, I, P, Z], I),
}

# constants of csrc/common.h and csrc/sstep.h the launchers' layouts depend on
K_MAX_BASIS = 64          # kMaxBasis: rec / coef hold kMaxBasis + 2 doubles, the Gram matrix (kMaxBasis + 1)^2
K_CANCEL_TOL = 1e-8       # kCancelTol
SSTEP_KR, SSTEP_KS = 8, 4
SSTEP_KTRI = SSTEP_KR * (SSTEP_KR + 1) // 2


def sstep_tri(r, c):
    """sstep::tri: packed upper triangle of the kR x kR dots, r <= c."""
    return r * SSTEP_KR - r * (r - 1) // 2 + (c - r)


class Launchers:
    """Attribute access to the launchers of one loaded library: ``Launchers(lib).v_dot(ctx.h, n, x, y, out)``."""

    def __init__(self, lib):
        for mangled, (name, argtypes, restype) in LAUNCHERS.items():
            f = getattr(lib, mangled)            # AttributeError: the symbol (= that signature) is gone
            f.argtypes, f.restype = argtypes, restype
            setattr(self, name, f)
