#!/usr/bin/env python3
"""Golden vectors for the MIA-2022 stage-2 batch body with the tree's DSCD criterion (CL_utils.CRD_loss_v2.CRDLoss over
ContrastMemory_v4: the import of "MIA 2022/train_test_path_multi_distill_v2.py":24-25), produced by importing and RUNNING the
reference's own modules where they lie, in the form of make_golden_mia2022_step.py: networks_new.define_net / define_optimizer,
KD_loss.DistillKL, the criterion, and the trainer's momentum_AEKD_loss / update_ema_variables (compiled from the trainer file
where it lies: the module itself imports dgl / torchvision, absent here).  Settings: --neg_reweight True, --select_pos_mode
hard, --nce_p 100, --nce_p2 20, --nce_k 512; three steps at B = 8, 64 x 64.  The criterion call is the trainer's
criterion(epoch / niter_decay, path_feat, t_feat.detach(), index, sample_idx) (:436-437) and returns a 0-d tensor: there is no
epoch weight on the CRD terms.

Conditions on the inputs, as in make_golden_dscd.py: every row of sample_idx is drawn WITHOUT replacement and stored in the
fixture; on the reference's own sort keys neighbouring keys of every row's positives differ by at least 2e-6 in every call of
every run; every weight 1 + (s_relation - t_relation) is positive.  A draw that misses a condition is skipped (next seed).

Build machine only.  Writes tests/golden/dscd_step_b8_h64.npz, dscd_step_warm_b8_h64.npz, dscd_step_b8_h64_fp64.npz."""
import contextlib
import io
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
import make_golden as MG   # noqa: E402

REF = os.path.join(os.path.dirname(MG.REF), "MIA 2022")
MIN_GAP = 2e-6
P, P2, K = 100, 20, 512


class Unfit(Exception):
    def __init__(self, step, msg):
        super().__init__(msg)
        self.step = step


def main():
    from make_golden import install_shims, npz
    install_shims()
    sys.path.insert(0, REF)
    os.chdir(REF)
    tmp = tempfile.mkdtemp()
    sys.argv = ["x", "--distill", "crd", "-a", "1", "-b", "0.02", "--num_teachers", "2", "--CE_grads",
                "--model_name", "golden", "--fixed_model", "t", "--reg_type", "none", "--beta1", "0.9",
                "--assign_weights", "True", "--cut_fuse_grad", "--input_size_omic", "320", "--dropout_rate", "0",
                "--gpu_ids", "-1", "--checkpoints_dir", tmp, "--nce_p", str(P), "--nce_p2", str(P2), "--nce_k", str(K),
                "--nce_k2", str(K), "--neg_reweight", "True", "--select_pos_mode", "hard", "--grads_m", "0.9",
                "--grads_thresh", "False"]
    with contextlib.redirect_stdout(io.StringIO()):
        import options
        opt = options.parse_args()
        import networks_new as NN
        from KD_loss import DistillKL
        import importlib
        dscd = importlib.import_module("CL_utils.CRD_loss_v2")
    assert opt.neg_reweight == "True" and opt.select_pos_mode == "hard" and opt.select_pos_pairs is True
    src = open(os.path.join(REF, "train_test_path_multi_distill_v2.py")).read()
    ns = {"torch": torch, "Variable": torch.autograd.Variable}
    for a, b in (("def momentum_AEKD_loss", "def AEKD_loss"), ("def update_ema_variables", "def train(")):
        s0 = src.index(a); s1 = src.index(b, s0)
        exec(compile(src[s0:s1], a + "<reference>", "exec"), ns)     # runs the reference's own function text
    momentum_AEKD_loss, update_ema_variables = ns["momentum_AEKD_loss"], ns["update_ema_variables"]

    from oracle import weights as W
    from oracle.losses import CRDState
    from oracle.step import synthetic_batch
    B, H, n_data = 8, 64, 1024

    def columns(index, seed):
        g = torch.Generator().manual_seed(seed)
        rows = []
        for b in range(index.shape[0]):
            perm = torch.randperm(n_data, generator=g)
            rows.append(torch.cat([index[b:b + 1], perm[perm != index[b]][:P + K - 1]]))
        return torch.stack(rows)

    def checked_call(crd, epoch_frac, path_feat, t_feat, index, sidx, what):
        """The trainer's criterion call, with the fixture's conditions checked on the reference's own tensors."""
        with torch.no_grad():
            v1, v2 = crd.embed_s(path_feat), crd.embed_t(t_feat)
            w1, w2 = crd.contrast.memory_v1[sidx], crd.contrast.memory_v2[sidx]
            s_rel = torch.bmm(w1 / w1.norm(dim=2, keepdim=True), (v1 / v1.norm(dim=1, keepdim=True)).unsqueeze(-1))
            t_rel = torch.bmm(w2 / w2.norm(dim=2, keepdim=True), (v2 / v2.norm(dim=1, keepdim=True)).unsqueeze(-1))
            wmin = float((s_rel - t_rel + 1)[:, P:].min())
        if wmin <= 0:
            raise Unfit(what[0], "step %d %s: weight %.3f" % (what + (wmin,)))
        seen = []
        _sort = torch.sort

        def rec_sort(x, *a, **k):
            out = _sort(x, *a, **k); seen.append((x.detach().clone(), out[1].clone())); return out
        torch.sort = rec_sort
        try:
            with contextlib.redirect_stdout(io.StringIO()):
                loss = crd(epoch_frac, path_feat, t_feat, index, sidx)
        finally:
            torch.sort = _sort
        keys, order = seen[-1]
        gap = float(np.diff(np.sort(keys.squeeze(-1).double().numpy(), axis=1), axis=1).min())
        if gap < MIN_GAP:
            raise Unfit(what[0], "step %d %s: neighbouring sort keys %.2e apart" % (what + (gap,)))
        sel = order.squeeze(-1)[:, :P2].clone()
        sel[:, 0] = 0
        return loss, sel.to(torch.int32), gap, wmin

    def run(dt, rec, base, warm=None, collect=False):
        with contextlib.redirect_stdout(io.StringIO()):
            student = NN.define_net(opt, 1, path_only=True)
            ema = NN.define_net(opt, 1, path_only=True)
            teacher = NN.define_net(opt, 1)
        student.load_state_dict(W.make_state_dict(W.student_shapes(), 1))
        ema.load_state_dict(W.make_state_dict(W.student_shapes(), 2))
        teacher.load_state_dict(W.make_state_dict(W.teacher_shapes(320), 3))
        for p in ema.parameters():
            p.detach_()
        for p in teacher.parameters():
            p.detach_(); p.requires_grad = False
        crds = []
        for i in range(2):
            torch.manual_seed(20 + i)
            with contextlib.redirect_stdout(io.StringIO()):
                c = dscd.CRDLoss(opt, n_data)
            c.embed_s.load_state_dict(W.make_state_dict(W.embed_shapes(), 10 + 2 * i))
            c.embed_t.load_state_dict(W.make_state_dict(W.embed_shapes(), 11 + 2 * i))
            st = CRDState(n_data, seed=20 + i)
            c.contrast.memory_v1.copy_(st.memory_v1); c.contrast.memory_v2.copy_(st.memory_v2)
            crds.append(c)
        ml = torch.nn.ModuleList([student, crds[0].embed_s, crds[0].embed_t, crds[1].embed_s, crds[1].embed_t])
        optimizer = NN.define_optimizer(opt, ml)
        import _warm
        wnames, wparams = _warm.param_names(student), list(ml.parameters())
        if warm is not None:
            _warm.set_torch_adam(optimizer, wnames, wparams, warm)
            NN.define_scheduler(opt, optimizer)     # the trainer's LambdaLR applies its epoch-0 factor on creation
            rec["lr"] = optimizer.param_groups[0]["lr"]
        kl = DistillKL(opt.kd_T)
        for mod in (student, ema, teacher, crds[0], crds[1]):
            mod.to(dt)
        ml.train(); teacher.train()
        scale, iter_num = None, (_warm.T0 if warm is not None else 0)
        epochs = [3, 3, 7]
        for it in range(3):
            bt = synthetic_batch(B, H, n_data=n_data, P=P, K=K, seed=300 + it)
            bt["sample_idx"] = columns(bt["index"], base[it])
            bt = {k: (v.to(dt) if v.dtype.is_floating_point else v) for k, v in bt.items()}
            epoch = epochs[it]
            _, path_feat, logit_path, pred_path, _ = student(x_path=bt["x_path"])
            with torch.no_grad():
                _, ema_path_feat, ema_logit_path, _, _ = ema(x_path=bt["ema_x_path"])
                fuse_feat, _, _, _, logits, pred, _, _, _, _, _ = teacher(x_path=bt["x_path"], x_omic=bt["x_omic"])
            loss_cls = torch.nn.functional.nll_loss(pred_path, bt["grade"])
            loss_div1 = kl(logit_path, logits[-1].detach())
            loss_div2 = kl(logit_path, ema_logit_path.detach())
            loss_kd1, sel1, gap1, wm1 = checked_call(crds[0], epoch / opt.niter_decay, path_feat, fuse_feat.detach(), bt["index"],
                                                     bt["sample_idx"], (it, "kd1"))
            loss_kd2, sel2, gap2, wm2 = checked_call(crds[1], epoch / opt.niter_decay, path_feat, ema_path_feat.detach(), bt["index"],
                                                     bt["sample_idx"], (it, "kd2"))
            assert loss_kd1.dim() == 0 and loss_kd2.dim() == 0
            loss_div1 = opt.alpha * loss_div1; loss_div2 = opt.alpha * loss_div2
            loss_kd1 = opt.beta * loss_kd1; loss_kd2 = opt.beta * loss_kd2
            kd_list = [loss_div1, loss_div2, loss_kd1, loss_kd2]
            scale, loss_KD = momentum_AEKD_loss(opt, optimizer, loss_cls, path_feat, kd_list, scale)
            if opt.grads_thresh == "False":
                loss_KD = loss_KD * len(kd_list)
            loss = opt.lambda_nll * loss_cls + loss_KD        # reg_type none: define_reg contributes 0
            if not bool(torch.isfinite(loss)):
                raise Unfit(it, "step %d: loss %r" % (it, loss))
            optimizer.zero_grad()
            loss.backward()
            if collect:
                return _warm.grad_scales(wnames, wparams, opt.weight_decay)
            if it == 0:
                rec.update(g0_conv1=student.conv1.weight.grad.clone(), g0_fc2_w=student.fc_new2.weight.grad.clone(),
                           g0_embed_s0=crds[0].embed_s.linear.weight.grad.clone(),
                           g0_embed_t1=crds[1].embed_t.linear.weight.grad.clone())
            optimizer.step()
            update_ema_variables(student, ema, opt.ema_decay, iter_num)
            iter_num += 1
            scale = scale.detach()
            sd = student.state_dict(); esd = ema.state_dict()
            rec.update({f"epoch{it}": epoch, f"sidx{it}": bt["sample_idx"], f"sel0_{it}": sel1, f"sel1_{it}": sel2,
                        f"min_gap{it}": min(gap1, gap2), f"min_weight{it}": min(wm1, wm2),
                        f"logit_path{it}": logit_path, f"path_feat{it}": path_feat,
                        f"ema_logit{it}": ema_logit_path, f"fuse_logit{it}": logits[-1], f"loss_cls{it}": loss_cls,
                        f"loss_div1_{it}": loss_div1, f"loss_div2_{it}": loss_div2, f"loss_kd1_{it}": loss_kd1,
                        f"loss_kd2_{it}": loss_kd2, f"scale{it}": scale.clone(), f"loss_KD{it}": loss_KD, f"loss{it}": loss,
                        f"p_fc2_{it}": sd["fc_new2.weight"].clone(), f"ema_fc2_{it}": esd["fc_new2.weight"].clone(),
                        f"bank0_v1_rows{it}": crds[0].contrast.memory_v1[bt["index"]].clone(),
                        f"bank1_v2_rows{it}": crds[1].contrast.memory_v2[bt["index"]].clone(),
                        f"params0_{it}": crds[0].contrast.params.clone()})
            print(str(dt), "step", it, "loss", float(loss), "scale", scale.tolist(), "gap %.2e weight %.3f" % (min(gap1, gap2), min(wm1, wm2)))

    import _warm
    base = [500, 600, 700]      # the seed of every step's sample_idx draw: a step that misses a condition in any run moves on
    for attempt in range(400):
        meta = dict(B=B, H=H, n_data=n_data, P=P, P2=P2, K=K, grads_m=opt.grads_m, niter_decay=opt.niter_decay, alpha=opt.alpha,
                    beta=opt.beta, sidx_seeds=np.array(base), min_gap=MIN_GAP)
        try:
            with contextlib.redirect_stdout(io.StringIO()):
                rec = dict(meta)
                run(torch.float32, rec, base)
                scales = run(torch.float32, {}, base, collect=True)
                recw = dict(meta)
                recw.update(_warm.pack_scales(scales)); recw["t0"] = _warm.T0
                run(torch.float32, recw, base, warm=scales)
                rec64 = {}
                run(torch.float64, rec64, base)
        except Unfit as e:
            print("sample_idx seeds %r: %s" % (base, e))
            base[e.step] += 1
            continue
        break
    else:
        raise SystemExit("no sample_idx seeds fit")
    print("sample_idx seeds", base, "losses", [float(rec["loss%d" % it]) for it in range(3)],
          "smallest key gap %.2e, smallest weight %.3f" % (min(rec["min_gap%d" % it] for it in range(3)),
                                                          min(rec["min_weight%d" % it] for it in range(3))))
    # step 0 (identical weights in every run): the float64 run selects the same positives.  Later steps run on Adam-updated weights
    # that differ between the runs by more than the keys' gaps
    for k in ("sel0_0", "sel1_0"):
        assert np.array_equal(npz(rec)[k], npz(rec64)[k]), k
    np.savez_compressed(os.path.join(HERE, "dscd_step_b8_h64.npz"), **npz(rec))
    recw = {k: v for k, v in recw.items() if not k.startswith(("path_feat", "g0_conv1"))}
    np.savez_compressed(os.path.join(HERE, "dscd_step_warm_b8_h64.npz"), **npz(recw))
    keep = ("logit_path", "path_feat", "ema_logit", "loss", "scale", "bank0", "bank1", "g0_conv1", "p_fc2", "ema_fc2")
    rec64 = {k: v for k, v in rec64.items() if k.startswith(keep)}
    np.savez_compressed(os.path.join(HERE, "dscd_step_b8_h64_fp64.npz"), **npz(rec64))
    print("written dscd_step_b8_h64{,_warm,_fp64}.npz")


if __name__ == "__main__":
    main()
