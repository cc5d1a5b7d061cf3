"""Drop-in for the reference's "MIA 2022/CL_utils/CRD_loss_v2.py": the DSCD criteria of the MIA-2022 tree ("Discrepancy
Supervised Contrastive Distillation"), the import of "MIA 2022/train_test_path_multi_distill_v2.py":24-25.
  CRDLoss     (:14-54)  over ContrastMemory_v4: positives ranked by teacher-minus-student discrepancy, every negative kept and,
              under --neg_reweight True, weighted by 1 + (student similarity - teacher similarity)
  CRDLoss_v2  (:57-103) over ContrastMemory_mono, the one-directional form: no embed_t, only the student receives a gradient
  ContrastLoss_v2 (:107-144; the formulas of CRD_loss.py), Embed (:148-162), Normalize (:165-174): the classes of CRD_loss.py
Inside the criteria the NCE arithmetic is fused into ph_crd_loss_grad / ph_crd_loss_grad_one."""
import torch.nn as nn

from .CRD_loss import ContrastLoss_v2, Embed, Normalize   # noqa: F401  (re-exported: same classes as CRD_loss_v2.py:107-174)
from .memory_new import ContrastMemory_v4, ContrastMemory_mono, check_feat_dim

eps = 1e-7


def _check_sample_kd(sample_KD):
    if sample_KD not in ("False", "True"):
        raise UnboundLocalError("local variable 'loss' referenced before assignment")   # what CRD_loss_v2.py:144 raises there


class CRDLoss(nn.Module):
    """CRD_loss_v2.py:14-54.  forward(epoch, f_s, f_t, idx, contrast_idx) -> 0-d loss s_loss + t_loss (the [B] per-sample losses
    with opt.sample_KD == "True"); contrast_idx is [B, nce_p + nce_k]."""

    def __init__(self, opt, n_data):
        super().__init__()
        check_feat_dim(opt.feat_dim)
        self.P = opt.nce_p
        self.P2 = opt.nce_p2
        self.embed_s = Embed(opt.s_dim, opt.feat_dim)
        self.embed_t = Embed(opt.t_dim, opt.feat_dim)
        self.contrast = ContrastMemory_v4(opt.feat_dim, n_data, opt.nce_p, opt.nce_k, opt.nce_t, opt.nce_m,
                                          opt.select_pos_pairs, opt.nce_p2, opt.select_neg_pairs,
                                          getattr(opt, "neg_reweight", "False"), opt.nce_k2)
        self.sample_KD = getattr(opt, "sample_KD", "False")
        self.contrast.sample_KD = self.sample_KD == "True"
        self.criterion_t = ContrastLoss_v2(n_data, sample_KD=self.sample_KD)
        self.criterion_s = ContrastLoss_v2(n_data, sample_KD=self.sample_KD)
        self.select_pos_mode = opt.select_pos_mode

    def forward(self, epoch, f_s, f_t, idx, contrast_idx=None, ranks=None):
        _check_sample_kd(self.sample_KD)
        f_s = self.embed_s(f_s)
        f_t = self.embed_t(f_t)
        return self.contrast.loss(epoch, f_s, f_t, idx, contrast_idx, self.select_pos_mode, ranks)


class CRDLoss_v2(nn.Module):
    """CRD_loss_v2.py:57-103, the one-directional criterion: the teacher's feature is used as it is (detached, L2-normalised:
    :95-98), so opt.t_dim must equal opt.feat_dim; the bank is called with (teacher, student) (:100) and the loss is
    criterion_s(out_s, P2) alone."""

    def __init__(self, opt, n_data):
        super().__init__()
        check_feat_dim(opt.feat_dim)
        if opt.t_dim != opt.feat_dim:
            raise ValueError("CRDLoss_v2 has no embed_t: t_dim %r must equal feat_dim %r (CRD_loss_v2.py:95-100)"
                             % (opt.t_dim, opt.feat_dim))
        self.P = opt.nce_p
        self.P2 = opt.nce_p2
        self.select_pos_mode = opt.select_pos_mode
        self.l2norm = Normalize(2)
        self.embed_s = Embed(opt.s_dim, opt.feat_dim)
        self.contrast = ContrastMemory_mono(opt.feat_dim, n_data, opt.nce_p, opt.nce_k, opt.nce_t, opt.nce_m,
                                            opt.select_pos_pairs, opt.nce_p2, opt.select_neg_pairs,
                                            getattr(opt, "neg_reweight", "False"), opt.nce_k2)
        self.sample_KD = getattr(opt, "sample_KD", "False")
        self.contrast.sample_KD = self.sample_KD == "True"
        self.criterion_s = ContrastLoss_v2(n_data, sample_KD=self.sample_KD)

    def forward(self, epoch, f_s, f_t, idx, contrast_idx=None, ranks=None):
        _check_sample_kd(self.sample_KD)
        f_t = self.l2norm(f_t.detach())
        f_s = self.embed_s(f_s)
        loss = self.contrast.loss(epoch, f_t, f_s, idx, contrast_idx, self.select_pos_mode, ranks)
        self.memory_t = self.contrast.memory_v1      # (:100 keeps the bank's second return value)
        return loss
