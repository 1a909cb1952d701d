"""Bitwise pin of the nine streaming passes built on csrc/stream.h (bk_fold_contract, bk_hopf_contract, bk_hopf_nf_rhs,
bk_hopf_nf_contract, bk_hopf_orbit, bk_nf1d_dots, bk_nf1d_rhs, bk_nf1d_contract, bk_nf1d_predict).

The sums of the reducing passes are promised bitwise reproducible; that property is the per-lane element order, the wave and
workgroup order and the grid size of the shared skeleton, which the accuracy bounds of the other tests (4 n eps sum |terms|) do
not see.  tests/golden/stream_pass_bits.json holds what the library computed BEFORE the passes were moved onto the shared
skeleton: every sum as float.hex(), every written vector as the SHA-256 of its bytes.  A key that is missing fails.

Inputs are exact integer arithmetic, ((i a + b) mod 1000003) / 1000003 - 0.5 with one (a, b) per stream, so they do not depend
on a random generator.  Cases: the smallest shapes that reach each branch of the skeleton --
  SH (n points, U = 2: chunks of 512 pairs): 3 (ragged item + odd tail), 4099 (four full chunks, a ragged item, odd tail; also 8
  bytes into the allocation and with ONE stream misaligned: element-by-element path), 2 100 231 (second grid-stride sweep at the
  kRedBlocks cap), 2^22 + 1031 (non-temporal loads);
  cGL (N points per field, U = 1: chunks of 256 pairs): 384 (below one chunk), 2624 (chunks + ragged end; also at offset 1), 391
  (odd: the second field is misaligned), 2050 x 1026 (N >= 2^21 and no multiple of 512: non-temporal, five sweeps, ragged end).

Re-record (only from a library whose sums are the reference):  BKHIP_LIB=<libbkhip.so> python tests/test_gpu_stream_pass_bits.py --record
"""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stream_pass_bits.json")
PRIME = 1000003
SH_PARS = [-0.7, 2.0]
CGL_PARS = dict(r=0.3, mu=0.1, nu=1.0, c3=-1.0, c5=1.0, gamma=0.2)
SH_CASES = [(3, "al"), (4099, "al"), (4099, "off"), (4099, "mis"), (2 * 1024 ** 2 + 3 * 1024 + 7, "al"), ((1 << 22) + 1031, "al")]
CGL_CASES = [((24, 16), "al"), ((64, 41), "al"), ((23, 17), "al"), ((64, 41), "off"), ((2050, 1026), "al")]
GROUPS = [f"sh-{n}-{lay}" for n, lay in SH_CASES] + [f"cgl-{d[0]}x{d[1]}-{lay}" for d, lay in CGL_CASES]


def _stream(k, n):
    """Stream k of n elements: exact in int64, one division in float64."""
    i = np.arange(n, dtype=np.int64)
    return ((i * (12347 + 7919 * k) + (101 + 1009 * k)) % PRIME).astype(np.float64) / PRIME - 0.5


class _Pool:
    """Streams 0..8 of length n on the device, aligned (offset 0) and 8 bytes into their allocation (offset 1).  layout "al":
    all aligned; "off": all misaligned; "mis": only the LAST stream a pass asks for is misaligned."""

    def __init__(self, ctx, n, layout):
        import torch
        from bk_amd import hip
        self.layout = layout
        self.v = {}
        for off in {"al": (0,), "off": (1,), "mis": (0, 1)}[layout]:
            for k in range(9):
                t = torch.empty(n + off, dtype=torch.float64, device=ctx.torch_device)[off:]
                t.copy_(torch.from_numpy(_stream(k, n)))
                self.v[k, off] = hip.HipVec(ctx, t)
                assert t.data_ptr() % 16 == 8 * off

    def __call__(self, *ks):
        off = [1 if self.layout == "off" else 0] * len(ks)
        if self.layout == "mis":
            off[-1] = 1
        return [self.v[k, o] for k, o in zip(ks, off)]


def _hex(*vals):
    out = []
    for v in vals:
        out += [float(v.real).hex(), float(v.imag).hex()] if isinstance(v, complex) else [float(v).hex()]
    return out


def _sha(*vecs):
    return [hashlib.sha256(v.numpy().tobytes()).hexdigest() for v in vecs]


def _sh_group(ctx, n, layout):
    from bk_amd import codim2, hip
    from bk_amd import normal_form1d as N1
    prob = hip.SwiftHohenberg1D(ctx, n, 6.0, lam=SH_PARS[0], nu=SH_PARS[1])
    S = _Pool(ctx, n, layout)
    small = n < 1 << 20
    out = {}
    for ip in (0, 1):
        for m in range(4):
            u, v, w, *X = S(*range(3 + m))
            sx, sp = codim2.fold_contract(prob, u, SH_PARS, ip, v, w, X)
            out[f"fold_contract/ip{ip}/m{m}"] = _hex(*sx, sp)
        u, z, zs = S(0, 1, 2)
        out[f"nf1d_dots/ip{ip}"] = _hex(*N1.nf1d_dots(prob, u, SH_PARS, ip, z, zs))
        u, z, zs, p, q = S(0, 1, 2, 3, 4)
        out[f"nf1d_contract/ip{ip}"] = _hex(*N1.nf1d_contract(prob, u, SH_PARS, ip, z, zs, p, q))
        # zeta* == zeta, the same device vector twice
        u, z = S(0, 1)
        out[f"nf1d_dots/ip{ip}/alias"] = _hex(*N1.nf1d_dots(prob, u, SH_PARS, ip, z, z))
        u, z, p, q = S(0, 1, 3, 4)
        out[f"nf1d_contract/ip{ip}/alias"] = _hex(*N1.nf1d_contract(prob, u, SH_PARS, ip, z, z, p, q))
        if small or ip == 1:
            u, z = S(0, 1)
            out[f"nf1d_rhs/ip{ip}"] = _sha(*N1.nf1d_rhs(prob, u, SH_PARS, ip, z, 0.375, -1.25))
    # predictor: every M with every choice of the optional streams; at the large sizes M = 4 with both and M = 2 with none
    coefs = [(0.5, -0.25, 1.5), (-0.5, 0.25, -1.5), (0.125, 3.0, -0.75), (-2.0, 0.0625, 0.3)]
    for M in range(1, 5):
        for hp in (True, False):
            for ht in (True, False):
                if not small and (M, hp, ht) not in ((4, True, True), (2, False, False)):
                    continue
                ks = [0, 1] + ([3] if hp else []) + ([5] if ht else [])
                x0, z, *rest = S(*ks)
                P = rest.pop(0) if hp else None
                T = rest.pop(0) if ht else None
                cs = [(a, b if hp else 0.0, c if ht else 0.0) for a, b, c in coefs[:M]]
                out[f"nf1d_predict/M{M}/p{int(hp)}t{int(ht)}"] = _sha(*N1.nf1d_predict(x0, z, P, T, cs))
    return out


def _cgl_group(ctx, dims, layout):
    from bk_amd import codim2, hip
    prob = hip.CGL2d(ctx, dims, (1.0, 1.0), **CGL_PARS)
    pv = [CGL_PARS[k] for k in prob.param_names]
    S = _Pool(ctx, 2 * dims[0] * dims[1], layout)
    out = {}
    for ip in (0, 1):
        for m in range(4):
            u, vr, vi, wr, wi, *X = S(*range(5 + m))
            s, P, Q = codim2.hopf_contract(prob, u, pv, ip, (vr, vi), (wr, wi), X)
            out[f"hopf_contract/ip{ip}/m{m}"] = _hex(*s, P, Q)
        u, zr, zi, sr, si, p, q, gr, gi = S(*range(9))
        out[f"hopf_nf_contract/ip{ip}"] = _hex(*codim2.hopf_nf_contract(prob, u, pv, ip, (zr, zi), (sr, si), p, q, (gr, gi)))
    u, zr, zi = S(0, 1, 2)
    (rr, ri), r11 = codim2.hopf_nf_rhs(prob, u, pv, (zr, zi))
    out["hopf_nf_rhs"] = _sha(rr, ri, r11)
    x0, zr, zi, p, q, gr, gi = S(*range(7))
    for M in (1, 8):
        ts = [0.3 + 0.77 * k for k in range(M)]
        out[f"hopf_orbit/M{M}"] = _sha(*codim2.hopf_orbit(x0, (zr, zi), p, q, (gr, gi), 0.01, 0.2, ts))
    return out


def _group(ctx, name):
    kind, size, layout = name.split("-")
    if kind == "sh":
        return _sh_group(ctx, int(size), layout)
    return _cgl_group(ctx, tuple(int(d) for d in size.split("x")), layout)


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("name", GROUPS)
def test_stream_pass_bits(ctx, golden, name):
    got = _group(ctx, name)
    assert len(got) >= 10
    bad = {k: (v, golden.get(f"{name}/{k}")) for k, v in got.items() if golden.get(f"{name}/{k}") != v}
    assert not bad, f"{len(bad)} of {len(got)} entries differ from (or are missing in) the recorded bits: {sorted(bad)[:8]}"


if __name__ == "__main__":
    assert sys.argv[1:] == ["--record"], "usage: BKHIP_LIB=<reference libbkhip.so> python tests/test_gpu_stream_pass_bits.py --record"
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from bk_amd import hip
    c = hip.Context(0)
    rec = {f"{g}/{k}": v for g in GROUPS for k, v in _group(c, g).items()}
    c.close()
    with open(GOLDEN, "w") as f:
        json.dump(rec, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"recorded {len(rec)} entries -> {GOLDEN}")
