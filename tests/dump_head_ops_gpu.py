"""Bit-for-bit acceptance of a refactor of the fp32 head and loss kernels (csrc/dense.hip, zoo.hip, zoo_rkd.hip, surv.hip) and of
their autograd glue (ops.py): every C entry of those files on seeded inputs at the edge shapes of the float64 sweeps
(tests/dense_emulation.py, tests/zoo_emulation.py, tests/test_gpu_survival.py), the raw output bytes written one file per call.
Run it once per build of the library, each in a fresh process, and compare the directories:
    python tests/dump_head_ops_gpu.py --out DIR_A
    PH_LIB_VARIANT=_parent python tests/dump_head_ops_gpu.py --out DIR_B
    python tests/dump_head_ops_gpu.py --compare DIR_A DIR_B        (no GPU needed; exit status 1 when any file differs)
    python tests/dump_head_ops_gpu.py --autograd OTHER_OPS_PY      (ops.py against another revision's ops.py, torch.equal)"""
import argparse
import filecmp
import importlib.util
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ACTS = (0, 1, 2, 3)        # PH_ACT_NONE / RELU / ELU / SIGMOID


def _rand(rs, *shape, scale=1.0):
    return torch.from_numpy((rs.standard_normal(shape) * scale).astype(np.float32)).cuda()


class Dump:
    def __init__(self, out):
        from multimodal_learning_amd._lib import lib, ptr, stream, check
        self.L, self.ptr, self.st, self.check = lib(), ptr, stream(), check
        self.out, self.names = out, []
        os.makedirs(out, exist_ok=True)

    def call(self, entry, *args):
        self.check(getattr(self.L, entry)(*args, self.st), entry)

    def save(self, name, *tensors):
        torch.cuda.synchronize()
        assert name not in self.names, name
        self.names.append(name)
        with open(os.path.join(self.out, name + ".bin"), "wb") as f:
            for t in tensors:
                f.write(t.detach().contiguous().cpu().numpy().tobytes())


def sgemm(d, rs):
    p = d.ptr
    for M, N, K in ((1, 1, 1), (17, 33, 129), (128, 128, 257), (130, 129, 65)):
        a, b, bias = _rand(rs, M, K), _rand(rs, K, N), _rand(rs, N)
        for a_kfast in (1, 0):
            A = a.contiguous() if a_kfast else a.t().contiguous()              # [M][K] or [K][M]
            sam, sak = (K, 1) if a_kfast else (1, M)
            for b_nfast in (1, 0):
                Bm = b.contiguous() if b_nfast else b.t().contiguous()         # [K][N] or [N][K]
                sbk, sbn = (N, 1) if b_nfast else (1, K)
                tag = "sgemm_%dx%dx%d_a%d_b%d" % (M, N, K, a_kfast, b_nfast)
                for act in ACTS:
                    c = torch.full((M, N), float("nan"), device="cuda")
                    d.call("ph_sgemm", p(A), p(Bm), p(bias), p(c), M, N, K, sam, sak, sbk, sbn, N, act, 0)
                    d.save("%s_act%d" % (tag, act), c)
                ldc = N + 3
                c = _rand(np.random.RandomState(M * 7 + N), M, ldc)
                d.call("ph_sgemm", p(A), p(Bm), None, p(c), M, N, K, sam, sak, sbk, sbn, ldc, 0, 1)
                d.save(tag + "_accumulate_ldc", c)
    for (M, N, K), nsplit in (((3, 5, 4097), 32), ((3, 5, 40), 4)):
        a, b, bias = _rand(rs, M, K), _rand(rs, K, N), _rand(rs, N)
        for a_kfast, b_nfast in ((1, 0), (0, 1)):
            A = a.contiguous() if a_kfast else a.t().contiguous()
            sam, sak = (K, 1) if a_kfast else (1, M)
            Bm = b.contiguous() if b_nfast else b.t().contiguous()
            sbk, sbn = (N, 1) if b_nfast else (1, K)
            for act in ACTS:
                c = torch.full((M, N), float("nan"), device="cuda")
                part = torch.zeros(nsplit * M * N, device="cuda")
                d.call("ph_sgemm_splitk", p(A), p(Bm), p(bias), p(c), p(part), nsplit, M, N, K, sam, sak, sbk, sbn, N, act)
                d.save("splitk_%dx%dx%d_n%d_a%d_b%d_act%d" % (M, N, K, nsplit, a_kfast, b_nfast, act), c)


def row_ops(d, rs):
    p = d.ptr
    for B in (1, 257):
        for C in (1, 3, 64):
            ys, yt1, yt2 = _rand(rs, B, C, scale=3.0), _rand(rs, B, C, scale=3.0), _rand(rs, B, C, scale=3.0)
            if C == 3:      # a teacher row whose smallest logit lies 500 (125 at T = 4) below its largest: p_t underflows to 0, the guard is taken
                yt1[B // 2] = torch.tensor([250.0, -250.0, 0.0])
            grade = torch.from_numpy(rs.randint(0, C, size=B).astype(np.int64)).cuda()
            g, gs, gb = _rand(rs, B, C), _rand(rs, 1), _rand(rs, B)
            inv_bnorm = 1.0 / max(B, 1)
            tag = "B%d_C%d" % (B, C)
            pred = torch.empty(B, C, device="cuda")
            d.call("ph_log_softmax", p(ys), p(pred), B, C)
            dx = torch.empty(B, C, device="cuda")
            d.call("ph_log_softmax_bwd", p(g), p(pred), p(dx), B, C)
            loss = torch.empty(1, device="cuda")
            d.call("ph_nll_fwd", p(pred), p(grade), p(loss), B, C, inv_bnorm)
            dpred = torch.empty(B, C, device="cuda")
            d.call("ph_nll_bwd", p(gs), p(grade), p(dpred), B, C, inv_bnorm)
            disc = torch.empty(B, device="cuda")
            d.call("ph_conf_discrepancy", p(ys), p(yt1), p(grade), p(disc), B, C, 2.0)
            total = torch.empty(1, device="cuda")
            d.call("ph_sum", p(ys), p(total), B * C, 0.5)
            d.save("rows_" + tag, pred, dx, loss, dpred, disc, total)
            for T in (1.0, 4.0):
                kl, dys = torch.empty(1, device="cuda"), torch.empty(B, C, device="cuda")
                d.call("ph_kl_fwd", p(ys), p(yt1), p(kl), B, C, T, inv_bnorm)
                d.call("ph_kl_bwd", p(gs), p(ys), p(yt1), p(dys), B, C, T, inv_bnorm)
                rows, drows = torch.empty(B, device="cuda"), torch.empty(B, C, device="cuda")
                d.call("ph_kl_rows_fwd", p(ys), p(yt1), p(rows), B, C, T)
                d.call("ph_kl_rows_bwd", p(gb), p(ys), p(yt1), p(drows), B, C, T)
                lp, losses, dl = torch.empty(B, C, device="cuda"), torch.empty(3, device="cuda"), torch.empty(3, B, C, device="cuda")
                d.call("ph_logit_losses", p(ys), p(yt1), p(yt2), p(grade), p(lp), p(losses), p(dl), B, C, T, inv_bnorm)
                d.save("kl_%s_T%g" % (tag, T), kl, dys, rows, drows, lp, losses, dl)


def dropout(d, rs):
    p = d.ptr
    ctr = torch.tensor([3], dtype=torch.int64, device="cuda")
    seed, off, P = 0x1234567, 4096, 0.25
    for n in (1, 257):
        x = _rand(rs, n)
        for alpha in (0, 1):
            outs = []
            y = x.clone(); d.call("ph_dropout", p(y), n, P, seed, off, alpha); outs.append(y)
            y = x.clone(); d.call("ph_dropout_dev", p(y), n, P, seed, off, p(ctr), alpha); outs.append(y)
            y = torch.empty(n, device="cuda"); d.call("ph_dropout_dev_to", p(x), p(y), n, P, seed, off, p(ctr), alpha); outs.append(y)
            y = x.clone(); d.call("ph_dropout_dev_to", p(y), p(y), n, P, seed, off, p(ctr), alpha); outs.append(y)
            y = x.clone(); d.call("ph_dropout_bwd_dev", p(y), n, P, seed, off, p(ctr), alpha); outs.append(y)
            y = torch.empty(n, device="cuda"); d.call("ph_dropout_bwd_dev_to", p(x), p(y), n, P, seed, off, p(ctr), alpha); outs.append(y)
            y = x.clone(); d.call("ph_dropout_bwd_dev_to", p(y), p(y), n, P, seed, off, p(ctr), alpha); outs.append(y)
            d.save("dropout_n%d_alpha%d" % (n, alpha), *outs)


def zoo(d, rs):
    p, L = d.ptr, d.L

    def ws(nbytes):
        return torch.zeros((nbytes + 3) // 4, device="cuda")
    for B, D in ((2, 3), (1030, 24)):
        fs, ft = _rand(rs, B, D).abs() + 0.1, _rand(rs, B, D).abs() + 0.1
        loss, dx, w = torch.empty(1, device="cuda"), torch.empty(B, D, device="cuda"), ws(L.ph_pkt_workspace_bytes(B, D))
        d.call("ph_pkt_loss_grad", p(fs), p(ft), p(loss), p(dx), B, D, p(w))
        d.save("pkt_%dx%d" % (B, D), loss, dx)
    for B, D in ((3, 3), (128, 128)):
        assert L.ph_rkd_one_workgroup_fits(B, D)
        fs, ft = _rand(rs, B, D), _rand(rs, B, D)
        loss, dx, w = torch.empty(1, device="cuda"), torch.empty(B, D, device="cuda"), ws(L.ph_rkd_workspace_bytes(B, D))
        d.call("ph_rkd_loss_grad", p(fs), p(ft), p(loss), p(dx), B, D, 25.0, 50.0, p(w))
        d.save("rkd_one_%dx%d" % (B, D), loss, dx)
    for Bg, D, lo, na in ((3, 2, 1, 2), (130, 200, 37, 70), (1024, 8, 1000, 24)):
        fs, ft = _rand(rs, Bg, D), _rand(rs, Bg, D)
        loss, dx, w = torch.empty(1, device="cuda"), torch.empty(Bg, D, device="cuda"), ws(L.ph_rkd_part_workspace_bytes(Bg, D, na))
        d.call("ph_rkd_loss_grad_part", p(fs), p(ft), Bg, D, lo, na, 25.0, 50.0, p(loss), p(dx), p(w))
        d.save("rkd_part_%dx%d_lo%d_na%d" % (Bg, D, lo, na), loss, dx)
    for B in (1, 4096):
        theta, t = _rand(rs, B), _rand(rs, B).abs()
        c = torch.from_numpy((rs.rand(B) < 0.7).astype(np.float32)).cuda()
        loss, dth = torch.empty(1, device="cuda"), torch.empty(B, device="cuda")
        d.call("ph_cox_loss_grad", p(theta), p(t), p(c), p(loss), p(dth), B)
        d.save("cox_%d" % B, loss, dth)


def survival(d, rs):
    p = d.ptr
    for B in (8, 300, 4096):
        ps, qs = [_rand(rs, B) for _ in range(3)], [_rand(rs, B) for _ in range(3)]
        t = _rand(rs, B).abs()
        c = torch.from_numpy((rs.rand(B) < 0.7).astype(np.float32)).cuda()
        for nt in (0, 1, 2, 3):
            terms, dg = torch.empty(9, device="cuda"), torch.empty(3, B, device="cuda")
            d.call("ph_surv_stage1_loss_grad", *map(p, ps + qs), p(t), p(c), B, nt, 0.7, 1.5, p(terms), p(dg))
            outs = [terms, dg]
            world, n = 2, B // 2
            gathered = torch.empty(world, 8, n, device="cuda")
            for r in range(world):
                sl = slice(r * n, (r + 1) * n)
                d.call("ph_surv_pack_rows", *[p(v[sl].contiguous()) for v in ps + qs + [t, c]], n, nt, p(gathered[r]))
            for r in range(world):
                terms, dg = torch.empty(9, device="cuda"), torch.empty(3, n, device="cuda")
                d.call("ph_surv_stage1_loss_grad_gathered", p(gathered), world, n, r, nt, 0.7, 1.5, p(terms), p(dg))
                outs += [terms, dg]
            d.save("surv_B%d_nt%d" % (B, nt), *outs)


def dump(out):
    d = Dump(out)
    for k, part in enumerate((sgemm, row_ops, dropout, zoo, survival)):
        part(d, np.random.RandomState(100 + k))
    print("%d calls dumped to %s (library: %s)" % (len(d.names), out, os.environ.get("PH_LIB_VARIANT", "") or "default"))


def compare(a, b):
    na, nb = sorted(os.listdir(a)), sorted(os.listdir(b))
    bad = sorted(set(na) ^ set(nb))
    _, mismatch, errors = filecmp.cmpfiles(a, b, sorted(set(na) & set(nb)), shallow=False)
    for n in sorted(set(na) & set(nb)):
        print("%-44s %s" % (n, "DIFFERS" if n in mismatch or n in errors else "equal"))
    print("%d files, %d differ, %d on one side only" % (len(set(na) | set(nb)), len(mismatch) + len(errors), len(bad)))
    return 1 if bad or mismatch or errors or not na else 0


class _OneRank:
    world_size, rank = 1, 0

    @staticmethod
    def all_gather_into(gathered, staging):
        gathered[0].copy_(staging)


def autograd(other_ops):
    """The autograd functions of ops.py against those of OTHER_OPS_PY on the same library: outputs and every input gradient"""
    import multimodal_learning_amd as m
    from multimodal_learning_amd import ops as new
    spec = importlib.util.spec_from_file_location(m.__name__ + "._ops_other", other_ops)
    old = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = old
    spec.loader.exec_module(old)
    assert old.__file__ != new.__file__
    rs = np.random.RandomState(7)
    rows, bad = [], 0

    def run(what, build, inputs):
        nonlocal bad
        res = []
        for mod in (new, old):
            xs = [x.clone().requires_grad_(True) if x is not None and x.is_floating_point() else x for x in inputs]
            outs = build(mod, xs)
            outs = outs if isinstance(outs, tuple) else (outs,)
            g = torch.autograd.grad(outs[0], [x for x in xs if x is not None and x.requires_grad],
                                    _rand(np.random.RandomState(11), *outs[0].shape) if outs[0].dim() else None)
            res.append([o.detach() for o in outs] + list(g))
        same = len(res[0]) == len(res[1]) and all(torch.equal(a, b) for a, b in zip(*res))
        bad += not same
        rows.append("%-40s %d tensors %s" % (what, len(res[0]), "equal" if same else "DIFFER"))

    B, K, N = 17, 129, 33
    x, w, b = _rand(rs, B, K), _rand(rs, N, K), _rand(rs, N)
    run("LinearFn", lambda mod, v: mod.LinearFn.apply(*v), [x, w, b])
    run("LinearFn (no bias)", lambda mod, v: mod.LinearFn.apply(v[0], v[1], None), [x, w])
    for act, name in ((new.ACT_NONE, "none"), (new.ACT_RELU, "relu"), (new.ACT_ELU, "elu")):
        run("LinearActFn " + name, lambda mod, v, act=act: mod.LinearActFn.apply(v[0], v[1], v[2], act), [x, w, b])
    x0, x1 = _rand(rs, B, 32), _rand(rs, B, 20)
    wc = _rand(rs, N, 32 + 1 + 20 + 1)
    run("CatLinearFn (two appended-one blocks)", lambda mod, v: mod.cat_linear([(v[2], True), (v[3], True)], v[0], v[1]), [wc, b, x0, x1])
    n = 300
    ps, qs = [_rand(rs, n, 1) for _ in range(3)], [_rand(rs, n, 1) for _ in range(3)]
    t, c = _rand(rs, n).abs(), torch.from_numpy((rs.rand(n) < 0.7).astype(np.float32)).cuda()
    for nt in (0, 3):
        run("SurvStage1LossFn nt=%d" % nt,
            lambda mod, v, nt=nt: mod.SurvStage1LossFn.apply(v[0], v[1], v[2], qs[0], qs[1], qs[2], t, c, nt, 0.7, 1.5), ps)
        run("SurvStage1GatheredFn nt=%d" % nt,
            lambda mod, v, nt=nt: mod.SurvStage1GatheredFn.apply(v[0], v[1], v[2], qs[0], qs[1], qs[2], t, c, nt, 0.7, 1.5, _OneRank,
                                                                 *mod.surv_gather_buffers(n, 1, "cuda")), ps)
    print("\n".join(rows))
    print("%d comparisons, %d differ" % (len(rows), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out")
    ap.add_argument("--compare", nargs=2, metavar="DIR")
    ap.add_argument("--autograd", metavar="OTHER_OPS_PY")
    a = ap.parse_args()
    if a.compare:
        sys.exit(compare(*a.compare))
    if a.autograd:
        sys.exit(autograd(a.autograd))
    dump(a.out)
