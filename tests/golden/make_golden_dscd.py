#!/usr/bin/env python3
"""Golden vectors of the DSCD criteria of the MIA-2022 tree, produced by importing and running the reference classes on the CPU
(build machine only; shims of make_golden.py): "MIA 2022/CL_utils/CRD_loss_v2.py" CRDLoss over ContrastMemory_v4 (neg_reweight
"True" and "False", `hard`; `mid` with the drawn ranks recorded) and CRDLoss_v2 over ContrastMemory_mono (`hard`), two consecutive
calls each (Z is set on the first, frozen on the second; the second scores against the momentum-updated banks), at B = 8,
P = 100, P2 = 20, K = 512, n_data = 1024, D = 128; plus one D = 64 and one D = 256 case at P = 12, P2 = 4, K = 40.

Saved per case and call: the inputs, the loss, d loss / d f_s, the gradients of the Embed layers, the selected columns (from the
reference's own torch.sort, intercepted), params (Z), the updated bank rows; the module's state_dict key / shape list; the same
calls in float64 (keys with the suffix _f64).

Conditions on the inputs (torch.sort is not stable, and a non-positive weight makes the reference's loss NaN - the goldens depend
on neither): every row's index columns are drawn WITHOUT replacement; on the reference's own sort keys, neighbouring keys of
every row's positives differ by at least 2e-6; every weight 1 + (s_relation - t_relation) is positive.  A seed that misses a
condition is skipped.

Usage:  python tests/golden/make_golden_dscd.py        # writes tests/golden/dscd_forward.npz
"""
import contextlib
import io
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG   # noqa: E402

REF = os.path.join(os.path.dirname(MG.REF), "MIA 2022")
MIN_GAP = 2e-6
# name -> (criterion, neg_reweight, mode, D, P, P2, K)
CASES = {
    "v4_rw_hard": ("CRDLoss", "True", "hard", 128, 100, 20, 512),
    "v4_plain_hard": ("CRDLoss", "False", "hard", 128, 100, 20, 512),
    "v4_rw_mid": ("CRDLoss", "True", "mid", 128, 100, 20, 512),
    "mono_hard": ("CRDLoss_v2", "False", "hard", 128, 100, 20, 512),
    "v4_rw_hard_d64": ("CRDLoss", "True", "hard", 64, 12, 4, 40),
    "mono_hard_d256": ("CRDLoss_v2", "False", "hard", 256, 12, 4, 40),
}
N_DATA, B, S_DIM = 1024, 8, 16      # (a narrow student feature keeps the Embed gradients, and the fixture, small)


class Unfit(Exception):
    pass


def case_opt(crit, rw, mode, D, P, P2, K):
    return types.SimpleNamespace(nce_p=P, nce_p2=P2, nce_k=K, nce_k2=K, nce_t=0.07, nce_m=0.5, feat_dim=D, s_dim=S_DIM,
                                 t_dim=D if crit == "CRDLoss_v2" else S_DIM, select_pos_pairs=True, select_neg_pairs="False",
                                 neg_reweight=rw, sample_KD="False", select_pos_mode=mode)


def draw_columns(g, y, width):
    """[B, width] bank rows, column 0 = y, no row twice within a sample."""
    rows = []
    for b in range(y.shape[0]):
        perm = torch.randperm(N_DATA, generator=g)
        perm = perm[perm != y[b]][:width - 1]
        rows.append(torch.cat([y[b:b + 1], perm]))
    return torch.stack(rows)


def run_case(mod, name, seed, dt):
    from oracle import weights as W
    from oracle.losses import CRDState
    crit, rw, mode, D, P, P2, K = CASES[name]
    opt = case_opt(*CASES[name])
    with contextlib.redirect_stdout(io.StringIO()):
        crd = getattr(mod, crit)(opt, N_DATA)
    crd.embed_s.load_state_dict(W.make_state_dict(W.embed_shapes(S_DIM, D), 10))
    if crit == "CRDLoss":
        crd.embed_t.load_state_dict(W.make_state_dict(W.embed_shapes(S_DIM, D), 11))
    st = CRDState(N_DATA, feat_dim=D, seed=21)
    crd.contrast.memory_v1.copy_(st.memory_v1); crd.contrast.memory_v2.copy_(st.memory_v2)
    rec = {"state_dict": np.array(["%s:%s" % (k, "x".join(map(str, v.shape))) for k, v in crd.state_dict().items()])}
    crd = crd.to(dt)
    g = torch.Generator().manual_seed(seed)
    ranks_all, sorts = [], []
    _choice, _sort = np.random.choice, torch.sort

    def rec_choice(*a, **k):
        r = _choice(*a, **k); ranks_all.append(np.asarray(r)); return r

    def rec_sort(x, *a, **k):
        out = _sort(x, *a, **k); sorts.append((x.detach().clone(), out[1].clone())); return out
    np.random.seed(11)
    for it in range(2):
        f_s = torch.randn(B, S_DIM, generator=g).to(dt).requires_grad_(True)
        f_t = torch.randn(B, opt.t_dim, generator=g).to(dt)
        y = torch.randperm(N_DATA, generator=g)[:B]
        idx = draw_columns(g, y, P + K)
        m1, m2 = crd.contrast.memory_v1.clone(), crd.contrast.memory_v2.clone()
        np.random.choice, torch.sort = rec_choice, rec_sort
        try:
            with contextlib.redirect_stdout(io.StringIO()):
                loss = crd(0.1, f_s, f_t, y, idx)
        finally:
            np.random.choice, torch.sort = _choice, _sort
        keys, order = sorts[-1]                        # [B, P, 1]: the reference's own keys (sorted descending) and its order
        ks = np.sort(keys.squeeze(-1).double().numpy(), axis=1)
        if float(np.diff(ks, axis=1).min()) < MIN_GAP:
            raise Unfit("%s call %d: neighbouring sort keys %.2e apart" % (name, it, float(np.diff(ks, axis=1).min())))
        ranks = torch.as_tensor(ranks_all[-1]) if mode == "mid" else torch.arange(P2)
        sel = order.squeeze(-1)[:, ranks].clone()
        sel[:, 0] = 0
        if crit == "CRDLoss":                          # the weights of the negatives (memory_new.py:460-464, :513-514)
            with torch.no_grad():
                v1, v2 = crd.embed_s(f_s), crd.embed_t(f_t)
                w1, w2 = m1[idx], m2[idx]
                s_rel = torch.bmm(w1 / w1.norm(dim=2, keepdim=True), (v1 / v1.norm(dim=1, keepdim=True)).unsqueeze(-1))
                t_rel = torch.bmm(w2 / w2.norm(dim=2, keepdim=True), (v2 / v2.norm(dim=1, keepdim=True)).unsqueeze(-1))
                wt = (s_rel - t_rel + 1)[:, P:, 0]
            if float(wt.min()) <= 0:
                raise Unfit("%s call %d: weight %.3f" % (name, it, float(wt.min())))
            rec["wmin%d" % it], rec["wmax%d" % it] = wt.min(), wt.max()
        if not bool(torch.isfinite(loss)):
            raise Unfit("%s call %d: loss %r" % (name, it, loss))
        ps = [crd.embed_s.linear.weight, crd.embed_s.linear.bias] + ([crd.embed_t.linear.weight] if crit == "CRDLoss" else [])
        gs = torch.autograd.grad(loss, [f_s] + ps)
        rec.update({"f_s%d" % it: f_s, "f_t%d" % it: f_t, "index%d" % it: y, "sidx%d" % it: idx, "loss%d" % it: loss,
                    "g_fs%d" % it: gs[0], "g_ws%d" % it: gs[1], "g_bs%d" % it: gs[2], "sel%d" % it: sel.to(torch.int32),
                    "params%d" % it: crd.contrast.params.clone(), "bank_v1_rows%d" % it: crd.contrast.memory_v1[y].clone(),
                    "bank_v2_rows%d" % it: crd.contrast.memory_v2[y].clone(), "min_gap%d" % it: np.diff(ks, axis=1).min()})
        if crit == "CRDLoss":
            rec["g_wt%d" % it] = gs[3]
    if mode == "mid":
        rec["ranks"] = np.stack(ranks_all)
    return rec


def main():
    MG.install_shims()
    sys.path.insert(0, REF)
    os.chdir(REF)
    with contextlib.redirect_stdout(io.StringIO()):
        import CL_utils.CRD_loss_v2 as mod
    out = dict(n_data=N_DATA, B=B, s_dim=S_DIM, T=0.07, momentum=0.5, bank_seed=21, min_gap=MIN_GAP,
               cases=np.array(list(CASES)))
    for name in CASES:
        crit, rw, mode, D, P, P2, K = CASES[name]
        out.update({name + ".crit": crit, name + ".neg_reweight": rw, name + ".mode": mode,
                    name + ".dims": np.array([D, P, P2, K])})
        for seed in range(77, 177):
            try:
                r32, r64 = run_case(mod, name, seed, torch.float32), run_case(mod, name, seed, torch.float64)
            except Unfit as e:
                print("seed %d skipped: %s" % (seed, e))
                continue
            for it in range(2):                        # the float64 run selects the same columns (the keys are MIN_GAP apart)
                assert np.array_equal(MG.npz(r32)["sel%d" % it], MG.npz(r64)["sel%d" % it]), (name, it)
            out[name + ".seed"] = seed
            out.update({"%s.%s" % (name, k): v for k, v in r32.items()})
            out.update({"%s.%s_f64" % (name, k): v for k, v in r64.items() if k[:-1] in (
                "loss", "g_fs", "g_ws", "g_bs", "g_wt", "params", "bank_v1_rows", "bank_v2_rows")})
            print("%s: seed %d, losses %.6f %.6f, smallest key gap %.2e" % (
                name, seed, float(r32["loss0"]), float(r32["loss1"]), min(float(r32["min_gap0"]), float(r32["min_gap1"]))))
            break
        else:
            raise SystemExit("no seed fits " + name)
    np.savez_compressed(os.path.join(HERE, "dscd_forward.npz"), **MG.npz(out))
    print("wrote dscd_forward.npz")


if __name__ == "__main__":
    main()
