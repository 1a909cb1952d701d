"""ctypes view of the launchers of the slab z-solve (``csrc/dct_slab.hip``), of the axis pass that runs its local transforms and
half passes (``csrc/dct_fast.hip``: ``dct_axis_fft``, ``dct_slab_half_ok``) and of the two host functions that fill its tables
(``csrc/dct.hip``: ``dct_twiddle_fill``, ``slab_tables_fill``), for the kernel tests -- the pattern of ``tests/stencil_abi.py``.

The library exports the launchers under their Itanium-mangled names.  A mangled name encodes the NAME of an argument struct, not
its layout: ``test_slab_zsolve_reference.py`` parses the two definitions of ``SlabK`` (``dct.hip``, ``dct_slab.hip``) and
``DctSlabHalf`` (``ops.h``) and compares them with the mirrors below.  ``rank`` and ``R`` are fields of ``SlabK`` and the half
passes take ``DctSlabHalf`` by pointer, so one process can play every rank.  ``include/bkhip.h`` stays the public ABI.
"""
import ctypes as C

import numpy as np

P, Z, I, D = C.c_void_p, C.c_size_t, C.c_int, C.c_double

# C type as written in the sources -> ctypes type (device pointers travel as raw addresses)
CTYPES = {"int": C.c_int, "size_t": C.c_size_t, "double": C.c_double, "bool": C.c_bool, "const double*": C.c_void_p,
          "double*": C.c_void_p}

# (field, C type, default member value or None) in declaration order
SLAB_K = [("nx", "int", None), ("ny", "int", None), ("nl", "int", None), ("R", "int", None), ("rank", "int", None),
          ("L", "size_t", None), ("Lr", "size_t", None), ("a", "double", None), ("shift", "double", None),
          ("lam0", "const double*", None), ("lam1", "const double*", None), ("lam_loc", "const double*", None),
          ("phi", "const double*", None)]
DCT_SLAB_HALF = [("face_y", "double*", "nullptr"), ("face_d", "const double*", "nullptr"), ("phi", "const double*", "nullptr"),
                 ("Lr", "size_t", 0), ("a", "double", 0.0), ("has_bottom", "bool", False), ("has_top", "bool", False)]
STRUCTS = {"SlabK": SLAB_K, "DctSlabHalf": DCT_SLAB_HALF}


def _mirror(name, table):
    names = {f for f, _, _ in table}

    def __init__(self, **kw):
        C.Structure.__init__(self)               # zero-initialised: every default member value of the two structs is a zero
        for f, v in kw.items():
            if f not in names:
                raise TypeError(f"{name} has no field {f}")
            setattr(self, f, v)
    return type(name, (C.Structure,), {"_fields_": [(f, CTYPES[t]) for f, t, _ in table], "__init__": __init__})


SlabK = _mirror("SlabK", SLAB_K)
DctSlabHalf = _mirror("DctSlabHalf", DCT_SLAB_HALF)

K_SLAB_MAX_FACES = 15            # kSlabMaxFaces (dct_slab.hip): R <= 16

# mangled name -> (short name, argtypes, restype).  SlabK goes by const reference (= a pointer); DctSplit, the dot count and
# DctFuse of dct_axis_fft are passed as null pointers here
LAUNCHERS = {
    "_ZN2bk17slab_faces_gatherEP6bk_ctxRKNS_5SlabKEPKdPd": ("slab_faces_gather", [P, C.POINTER(SlabK), P, P], I),
    "_ZN2bk16slab_faces_solveEP6bk_ctxRKNS_5SlabKEPKdPd": ("slab_faces_solve", [P, C.POINTER(SlabK), P, P], I),
    "_ZN2bk18slab_faces_correctEP6bk_ctxRKNS_5SlabKEPKdPd": ("slab_faces_correct", [P, C.POINTER(SlabK), P, P], I),
    "_ZN2bk12dct_axis_fftEP6bk_ctxiiiiiPKdS3_PdS3_S3_S3_diPKNS_8DctSplitEPiPKNS_7DctFuseEPKNS_11DctSlabHalfE":
        ("dct_axis_fft", [P, I, I, I, I, I, P, P, P, P, P, P, D, I, P, P, P, C.POINTER(DctSlabHalf)], I),
    "_ZN2bk16dct_slab_half_okEP6bk_ctxiiiPKdS3_": ("dct_slab_half_ok", [P, I, I, I, P, P], C.c_bool),
    "_ZN2bk16dct_twiddle_fillEiPd": ("dct_twiddle_fill", [I, P], Z),
    "_ZN2bk16slab_tables_fillEidPdS0_": ("slab_tables_fill", [I, D, P, P], None),
}


class Launchers:
    """Attribute access to the launchers of one loaded library: ``Launchers(lib).slab_faces_solve(ctx.h, byref(K), rbuf, out)``."""

    def __init__(self, lib):
        for mangled, (name, argtypes, restype) in LAUNCHERS.items():
            f = getattr(lib, mangled)            # AttributeError: the symbol (= that signature) is gone
            f.argtypes, f.restype = argtypes, restype
            setattr(self, name, f)

    def twiddle_table(self, N):
        """The host table of dct_twiddle_fill (count query, then the fill into an array poisoned with NaN)."""
        count = self.dct_twiddle_fill(N, None)
        tw = np.full(count, np.nan)
        assert self.dct_twiddle_fill(N, tw.ctypes.data) == count
        return tw

    def slab_tables(self, nl, az):
        """(lam_loc[nl], phi[2][nl]) of slab_tables_fill."""
        lam, phi = np.full(nl, np.nan), np.full((2, nl), np.nan)
        self.slab_tables_fill(nl, az, lam.ctypes.data, phi.ctypes.data)
        return lam, phi
