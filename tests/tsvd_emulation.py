"""A numpy float32 restatement of the tiled t-SVD prox (csrc/tsvd.hip, 128 < B <= 512): block one-sided Jacobi with the
kernel's block width, its round robin over the blocks and over the 32 columns of a block pair, its rotation, stopping
rule, column floor, `keep` rule and finish (T = D A^H X, Y = A T, inverse DFT).  It is not bit-exact with the device (numpy
sums pairwise, the kernel over lanes), it is the same algorithm in the same number format: its error against the float64
oracle (oracle/variants.py:update_aux) is what the algorithm costs, and the device is held to a multiple of it
(tests/test_gpu_tsvd_tiled.py).

Running the module writes tests/golden/tsvd_tiled_restatement.json: per shape the restatement's error and the sweeps every
frequency slice took (minutes at 512 rows, which is why the tests read the file instead of running it):
    python tests/tsvd_emulation.py
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

W = 16                      # TT_W: columns of a block
NC = 2 * W                  # columns a workgroup rotates
TB_TOL2 = np.float32(1e-12)
TB_MAX_SWEEPS = 30
TSVD_MAX_ROWS = 512
RECORD = os.path.join(ROOT, "tests", "golden", "tsvd_tiled_restatement.json")

# (B, V, D, tau): the first size past the single-workgroup kernels, an odd B, a padded and an exact block count, every V,
# the full LDS footprint
SHAPES = [(129, 2, 32, 0.1), (160, 4, 32, 0.3), (256, 4, 128, 0.3), (257, 6, 32, 0.05), (511, 4, 32, 0.5),
          (512, 4, 128, 0.3), (512, 8, 32, 0.02)]
MARGIN = 4.0
# 4 x the largest excess of the device's error over MARGIN x the restatement's that an MI355X run of
# tests/test_gpu_tsvd_tiled.py printed: "aux" in units of max(max |ref|, 1), "tnn" relative.  See that module's docstring.
# The run showed no excess at any shape (the device is closer to the oracle than this restatement), hence the zeros.
FLOOR = {"aux": 0.0, "tnn": 0.0}
DEFECTS = ("last_block", "skip_pair", "sigma2", "noconj")


def key(B, V, D, tau):
    return f"{B}x{V}x{D}@{tau:g}"


def make_stack(B, V, D):
    """The inputs of tests/test_gpu_losses.py::test_tsvd_update_aux_vs_oracle: row-normalised Gram matrices of ReLU'd
    normal features.  Returns a float32 torch tensor [B, B, V]."""
    import torch
    from oracle import variants as OV
    rng = np.random.default_rng(B * 10 + V)
    feats = [torch.tensor(rng.standard_normal((B, D)).clip(0), dtype=torch.float32) for _ in range(V)]
    return torch.stack(OV.update_adj_tensor(feats), dim=2)


def _rr(n, step):
    """Round robin of the kernels: pair i of step `step` over n players (player n - 1 stays)."""
    i = np.arange(n // 2)
    p = np.where(i == 0, n - 1, (step + i - 1) % (n - 1))
    q = (step + n - 2 - i) % (n - 1)
    return p, q


def _twiddle(k, v, V):
    ang = np.float32(2.0) * np.float32((k * v) % V) / np.float32(V)
    return np.float32(np.cos(np.pi * np.float64(ang))), np.float32(np.sin(np.pi * np.float64(ang)))


def _jacobi(A, B, col_floor, defect):
    """A: [S, ncol, B] complex64, column j of frequency slice k in A[k, j]; col_floor: [S].  Rotates in place; returns the
    sweeps every slice took.  The slices are independent and only share the numpy calls: a slice whose last sweep rotated
    nothing is left alone from then on, as the step launches of the kernel return at once for it."""
    S, ncol = A.shape[0], A.shape[1]
    nb = ncol // W
    last = (B - 1) // W if B % W else -1          # the partial block
    one = np.float32(1.0)
    floor = np.asarray(col_floor, dtype=np.float32)[:, None, None]
    active = np.ones(S, dtype=bool)
    sweeps = [0] * S
    for _ in range(TB_MAX_SWEEPS):
        if not active.any():
            break
        live = np.nonzero(active)[0]
        for k in live:
            sweeps[k] += 1
        rotated = np.zeros(S, dtype=bool)
        for t in range(nb - 1):
            bp, bq = _rr(nb, t)
            lo, hi = np.minimum(bp, bq), np.maximum(bp, bq)
            if defect == "skip_pair":
                m = ~((lo == 0) & (hi == 1))
                lo, hi = lo[m], hi[m]
            idx = np.concatenate([lo[:, None] * W + np.arange(W), hi[:, None] * W + np.arange(W)], axis=1)   # [np, 32]
            Wk = A[live][:, idx]                                                                         # [L, np, 32, B]
            moved = np.zeros(Wk.shape[:2], dtype=bool)
            for s in range(NC - 1):
                p, q = _rr(NC, s)
                a, b = Wk[:, :, p], Wk[:, :, q]                                                          # [L, np, 16, B]
                al = np.sum(a.real * a.real + a.imag * a.imag, axis=3, dtype=np.float32)
                be = np.sum(b.real * b.real + b.imag * b.imag, axis=3, dtype=np.float32)
                g = np.sum(np.conj(a) * b, axis=3, dtype=np.complex64)                                   # conj(a_p) . a_q
                g2 = g.real * g.real + g.imag * g.imag
                rot = (np.minimum(al, be) > floor[live]) & (g2 > TB_TOL2 * al * be)
                if defect == "last_block":
                    rot &= ((idx[:, p] // W != last) & (idx[:, q] // W != last))[None]
                if not rot.any():
                    continue
                sel = np.nonzero(rot)                                                                    # only the pairs that rotate
                a_s, b_s, al_s, be_s, g_s = a[sel], b[sel], al[sel], be[sel], g[sel]                     # [n, B], [n]
                rg = one / np.sqrt(g2[sel], dtype=np.float32)
                ze = (be_s - al_s) * (np.float32(0.5) * rg)
                tt = np.copysign(one, ze) / (np.abs(ze) + np.sqrt(one + ze * ze, dtype=np.float32))
                c = one / np.sqrt(one + tt * tt, dtype=np.float32)
                sn = c * tt
                e = (g_s * rg).astype(np.complex64)                                                      # e^{i phi}
                c, sn, e = c[:, None], sn[:, None], e[:, None]
                ea = e if defect == "noconj" else np.conj(e)
                a[sel] = (c * a_s - (sn * ea) * b_s).astype(np.complex64)
                b[sel] = (c * b_s + (sn * e) * a_s).astype(np.complex64)
                Wk[:, :, p] = a
                Wk[:, :, q] = b
                moved |= rot.any(axis=2)
            for li, k in enumerate(live):
                if moved[li].any():
                    A[k, idx[moved[li]]] = Wk[li, moved[li]]
                    rotated[k] = True
        active &= rotated
    return sweeps


def restate(adj, tau, defect=None):
    """adj [B, B, V] float32 -> (aux [B, B, V] float32, TNN, sweeps per frequency slice)."""
    assert defect in (None,) + DEFECTS
    adj = np.asarray(adj, dtype=np.float32)
    B, _, V = adj.shape
    tau = np.float32(tau)
    nb = ((B + W - 1) // W + 1) & ~1
    S = V // 2 + 1
    Xs, floors = [], []
    As = np.zeros((S, nb * W, B), np.complex64)
    for k in range(S):
        re = np.zeros((B, B), np.float32)
        im = np.zeros((B, B), np.float32)
        for v in range(V):
            c, s = _twiddle(k, v, V)
            re += adj[:, :, v] * c
            im -= adj[:, :, v] * s
        Xs.append((re + 1j * im).astype(np.complex64))
        floors.append(np.float32(1e-14) * np.sum(re * re + im * im, dtype=np.float32))
        As[k, :B] = Xs[k].T
    sweeps = _jacobi(As, B, floors, defect)
    ys, tnn_k = [], []
    for k in range(S):
        A, X, col_floor = As[k], Xs[k], floors[k]
        a2 = np.sum(A.real * A.real + A.imag * A.imag, axis=1, dtype=np.float32)
        sig = a2 if defect == "sigma2" else np.sqrt(a2, dtype=np.float32)
        keep = (a2 > np.float32(100.0) * col_floor) & (sig > tau)
        safe = np.where(keep, sig, np.float32(1.0))
        d = np.where(keep, (np.float32(1.0) - tau / safe) / np.where(keep, a2, np.float32(1.0)), np.float32(0.0)).astype(np.float32)
        tnn_k.append(np.sum(np.where(keep, sig - tau, np.float32(0.0)), dtype=np.float32))
        T = (d[:, None] * (np.conj(A) @ X)).astype(np.complex64)      # D A^H X
        ys.append((A.T @ T).astype(np.complex64))                     # A T
    aux = np.zeros((B, B, V), np.float32)
    for v in range(V):
        acc = ys[0].real + (np.float32(-1.0) if v & 1 else np.float32(1.0)) * ys[V // 2].real
        for k in range(1, V // 2):
            c, s = _twiddle(k, v, V)
            acc = acc + np.float32(2.0) * (ys[k].real * c - ys[k].imag * s)
        aux[:, :, v] = acc / np.float32(V)
    t = tnn_k[0] + tnn_k[V // 2]
    for k in range(1, V // 2):
        t = t + np.float32(2.0) * tnn_k[k]
    return aux, float(t / np.float32(V)), sweeps


def errors(aux, tnn, ref, tnn_ref):
    """(max |aux - ref|, |tnn - tnn_ref| / max(|tnn_ref|, 1))"""
    return (float(np.abs(np.asarray(aux, dtype=np.float64) - ref).max()),
            abs(float(tnn) - float(tnn_ref)) / max(abs(float(tnn_ref)), 1.0))


def record():
    with open(RECORD) as f:
        return json.load(f)


def tolerances(rec):
    """(aux tolerance, relative TNN tolerance) the device is held to at a recorded shape."""
    return (MARGIN * rec["aux_err"] + FLOOR["aux"] * max(rec["max_ref"], 1.0), MARGIN * rec["tnn_rel"] + FLOOR["tnn"])


def main():
    import time
    from oracle import variants as OV
    out = {}
    for B, V, D, tau in SHAPES:
        t0 = time.time()
        adj = make_stack(B, V, D)
        ref, tnn_ref = OV.update_aux(adj, tau)
        aux, tnn, sweeps = restate(adj.numpy(), tau)
        ea, et = errors(aux, tnn, ref, tnn_ref)
        out[key(B, V, D, tau)] = dict(aux_err=ea, tnn_rel=et, max_ref=float(np.abs(ref).max()), tnn_ref=float(tnn_ref),
                                      sweeps=sweeps)
        print(key(B, V, D, tau), out[key(B, V, D, tau)], "%.1f s" % (time.time() - t0), flush=True)
        with open(RECORD, "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
