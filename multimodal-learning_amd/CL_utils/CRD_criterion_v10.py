"""Drop-in for the reference's "MIA 2023/stage2_unimodal_student/CL_utils/CRD_criterion_v10.py" (SURVEY row a18),
`pos_extra == "neighbors"` (the shipped train_20230805.sh): CRD bank whose positives are the num_pos same-class
nearest neighbours (cosine) of the query's own bank row, weighted by their similarity, with per-sample loss weights.

The reference copies both banks to the host and calls sklearn's cosine_similarity + two torch.sort over n_data per
query every step (:72-79,110-116); here `ph_crd_bank_topk` scans the bank on the GPU.
`pos_extra == "centers"` with nce_p == 2 (:81-101: the positives are the MEAN bank row of the query's class and the query's
own row, the other classes' means join the negatives) is built: `ph_crd_class_centers` writes the class means behind the
bank and the same fused kernels run over the extended column lists.  nce_p > 2 clusters every class with sklearn KMeans
from a random initialisation at every call (:90-92, :126-128) - not reproducible, so with the default
`opt.centers_kmeans == "sklearn"` it raises.  `opt.centers_kmeans = "device"` (3 <= nce_p <= 9) runs a deterministic k-means of
this project's own instead, `ph_crd_kmeans_centers`: farthest-point initialisation, `opt.kmeans_iters`
(default 16) Lloyd iterations on the device, the nce_p - 1 centres of every class behind the bank rows.  It is not sklearn's
k-means++ and claims no draw parity; on a bank whose clustering is not in doubt it gives the reference's numbers
(tests/golden/make_golden_mia2023_kmeans.py)."""
import os

import numpy as np
import torch
import torch.nn as nn

from .CRD_loss import Embed, Normalize   # noqa: F401
from .memory_new import ContrastBank, CrdCall, _CRDCoreFn, check_feat_dim
from .._lib import lib, check, ptr, stream

eps = 1e-7


class ContrastMemory(ContrastBank):
    """CRD_criterion_v10.py:20-43: params = [K, T, Z_v1, Z_v2, momentum] + the class of every bank row.  The list widths are
    per call (CRDLoss.neighbor_columns / center_columns)."""

    def __init__(self, inputSize, outputSize, train_class_idx, K, T=0.07, momentum=0.5):
        super().__init__(inputSize, outputSize, K, T, momentum)
        self.class_idx = train_class_idx
        labels = torch.zeros(outputSize, dtype=torch.int32)
        for c, members in enumerate(train_class_idx):
            labels[torch.as_tensor(np.asarray(members)).long()] = c
        self.register_buffer("all_sample_labels", labels, persistent=False)
        self.center_k = 1          # centre rows per class behind the bank (CRDLoss sets nce_p - 1)

    def ensure_center_rows(self, dev):
        """`pos_extra == "centers"`: re-home both banks into allocations with len(class_idx) * center_k extra rows behind the
        n_data bank rows (the buffers stay [n_data, D] views, so state_dict / load_state_dict are unchanged) and build
        the flat class-member lists once.  Module.to() / .cuda() replace the buffers by compact copies; the next call
        re-homes them."""
        C = len(self.class_idx)
        n, D, ck = self.nLem, self.memory_v1.shape[1], self.center_k
        for name in ("memory_v1", "memory_v2"):
            ext = getattr(self, "_ext_" + name, None)
            cur = getattr(self, name)
            if ext is None or ext.device != cur.device or cur.data_ptr() != ext.data_ptr() or ext.shape[0] != n + C * ck:
                ext = torch.zeros(n + C * ck, D, device=cur.device, dtype=torch.float32)
                ext[:n].copy_(cur)
                setattr(self, "_ext_" + name, ext)
                self._buffers[name] = ext[:n]
        if getattr(self, "_members", None) is None or self._members.device != dev:
            lists = [np.asarray(m).astype(np.int32).reshape(-1) for m in self.class_idx]
            off = np.zeros(C + 1, dtype=np.int32)
            off[1:] = np.cumsum([len(x) for x in lists])
            cat = np.concatenate(lists) if off[-1] else np.zeros(1, dtype=np.int32)
            self._members = torch.as_tensor(cat, device=dev)
            self._member_off = torch.as_tensor(off, device=dev)
            self._max_class = int(max(len(x) for x in lists))
            self._center_ws = torch.empty(lib().ph_crd_class_centers_workspace_bytes_w(C, self._max_class, D), device=dev,
                                          dtype=torch.uint8)
            self._others = torch.as_tensor([[j for j in range(C) if j != c] for c in range(C)], device=dev, dtype=torch.int64)
            self._kmeans_ws = None
        if ck > 1 and (getattr(self, "_kmeans_ws", None) is None or self._kmeans_ws.device != dev):
            self._kmeans_ws = torch.empty(lib().ph_crd_kmeans_centers_workspace_bytes(C, self._max_class, ck), device=dev,
                                          dtype=torch.uint8)


class CRDLoss(nn.Module):
    """CRD_criterion_v10.py:180-239: forward(sample_weights, f_s, f_t, batch_label, idx, contrast_idx)
    -> (loss, sample_loss[B])."""

    MAX_NEIGHBORS = 64      # num_pos range of ph_crd_bank_topk (include/pathomic_hip.h)

    def __init__(self, opt, n_data, train_class_idx):
        super().__init__()
        check_feat_dim(opt.feat_dim)
        self.embed_s = Embed(opt.s_dim, opt.feat_dim)
        self.embed_t = Embed(opt.t_dim, opt.feat_dim)
        self.contrast = ContrastMemory(opt.feat_dim, n_data, train_class_idx, opt.nce_k, opt.nce_t, opt.nce_m)
        self.num_pos = opt.nce_p
        self.pos_extra = opt.pos_extra
        if self.pos_extra not in ("neighbors", "centers"):
            raise NotImplementedError("pos_extra '%s' (CRD_criterion_v10.py knows 'neighbors' and 'centers')" % self.pos_extra)
        if self.pos_extra == "neighbors" and not 1 <= self.num_pos <= self.MAX_NEIGHBORS:
            raise ValueError("pos_extra 'neighbors' with nce_p %d: outside 1 .. %d (ph_crd_bank_topk selects up to %d "
                             "neighbours per query and bank)" % (self.num_pos, self.MAX_NEIGHBORS, self.MAX_NEIGHBORS))
        if self.pos_extra == "neighbors" and self.num_pos > n_data:
            # (a bank of fewer rows leaves empty KNN slots - row 0x7fffffff, similarity -inf - that the column lists cannot hold)
            raise ValueError("pos_extra 'neighbors' with nce_p %d over a bank of %d rows: nce_p must not exceed n_data"
                             % (self.num_pos, n_data))
        self.centers_kmeans = getattr(opt, "centers_kmeans", "sklearn")
        self.kmeans_iters = int(getattr(opt, "kmeans_iters", 16))
        if self.pos_extra == "centers" and self.num_pos != 2:
            if self.centers_kmeans != "device":
                raise NotImplementedError("pos_extra 'centers' with nce_p %d: nce_p > 2 runs sklearn KMeans from a random "
                                          "initialisation per class and call (:90-93) - not reproducible, parity-unpinned; "
                                          "nce_p == 2 (class means) is built, and centers_kmeans=\"device\" runs the "
                                          "deterministic device k-means for 3 <= nce_p <= 9" % self.num_pos)
            if opt.feat_dim != 128:
                raise NotImplementedError("centers_kmeans 'device' with feat_dim %d: the device k-means is built for feat_dim 128 "
                                          "alone" % opt.feat_dim)
            if not 3 <= self.num_pos <= 9:
                raise NotImplementedError("pos_extra 'centers' with centers_kmeans 'device': nce_p %d outside 3 .. 9 (the "
                                          "device k-means holds 2 .. 8 centres per class)" % self.num_pos)
            if self.kmeans_iters < 1:
                raise ValueError("kmeans_iters must be >= 1, got %d" % self.kmeans_iters)
            small = [c for c, members in enumerate(train_class_idx) if len(members) < self.num_pos - 1]
            if small:      # sklearn: "n_samples=.. should be >= n_clusters=.."
                raise ValueError("pos_extra 'centers' with nce_p %d: class(es) %s have fewer than %d rows (n_samples should be "
                                 ">= n_clusters)" % (self.num_pos, small, self.num_pos - 1))
            self.contrast.center_k = self.num_pos - 1
        self.criterion_t = ContrastLoss_v2(n_data)
        self.criterion_s = ContrastLoss_v2(n_data)
        self._scan_override = os.environ.get("PH_CRD_SCAN")      # (read once: the numerics do not follow later changes)

    def forward(self, sample_weights, f_s, f_t, batch_label, idx, contrast_idx=None):
        mem = self.contrast
        if contrast_idx is None or contrast_idx.shape[1] != mem.K + 1:
            raise RuntimeError("contrast_idx must be [B, nce_k + 1]")
        v1 = self.embed_s(f_s)
        v2 = self.embed_t(f_t)
        B, D = v1.shape
        dev = v1.device
        contrast_idx = contrast_idx.contiguous()
        batch_label = batch_label.to(dev).long().contiguous()
        if self.pos_extra == "centers":
            call, knn = self.center_columns(B, D, batch_label, contrast_idx), {}
        else:
            call, knn = self.neighbor_columns(B, D, batch_label, contrast_idx)
        rows = _CRDCoreFn.apply(v1, v2, mem, idx, call)                      # [B]: (s + t) sample losses / bsz
        mem.last.update(knn)
        return _weighted(sample_weights, rows, mem, B)

    SCAN_MIN_ROWS = 8192

    @staticmethod
    def scan_negatives(K, n_data, override="env"):
        """Bank-scan form of the negatives when every bank row is drawn about once per query or more (K >= n_data) AND the bank
        is large (>= SCAN_MIN_ROWS rows: BASELINE configs[4] read as 65 536 negatives per query over the 65 536-row bank); the
        gathered kernels otherwise - in particular for the shipped command (nce_k 4096 over a bank of 1-2 k rows,
        train_20230805.sh:3-6), which keeps the summation order and the feature set (outputs_only, ranked selection) of the
        gathered form.  `override` "0" / "1" forces one form (tests, A/B); the default reads PH_CRD_SCAN from the
        environment - a CRDLoss instance reads it ONCE, at construction."""
        if override == "env":
            override = os.environ.get("PH_CRD_SCAN")
        if override in ("0", "1"):
            return override == "1"
        return K >= n_data and n_data >= CRDLoss.SCAN_MIN_ROWS

    def neighbor_columns(self, B, D, batch_label, contrast_idx):
        """`pos_extra == "neighbors"` (:72-80, :110-117): the num_pos same-class nearest bank rows of every query in either
        bank (ph_crd_bank_topk) in front of the K sampled negatives.  -> (the CrdCall of the fused CRD kernels: a column list
        per bank, the similarity weights of the positives; the KNN tensors); shared by forward() and the closed-form loss head
        (loss_head.FusedMia2023LossFn)."""
        mem = self.contrast
        NP, K = self.num_pos, mem.K
        dev = contrast_idx.device
        nb1 = torch.empty(B, NP, device=dev, dtype=torch.int64); nb2 = torch.empty_like(nb1)
        sim1 = torch.empty(B, NP, device=dev, dtype=torch.float32); sim2 = torch.empty_like(sim1)
        ws = torch.empty(lib().ph_crd_bank_topk_workspace_bytes_np(B, mem.nLem, NP), device=dev, dtype=torch.uint8)
        check(lib().ph_crd_bank_topk(ptr(mem.memory_v1), ptr(mem.memory_v2), ptr(mem.all_sample_labels),
                                     ptr(contrast_idx), K + 1, ptr(batch_label), B, mem.nLem, NP, D, ptr(nb1),
                                     ptr(nb2), ptr(sim1), ptr(sim2), ptr(ws), stream()), "ph_crd_bank_topk")
        if self.scan_negatives(K, mem.nLem, self._scan_override):
            # nce_k at or above the number of bank rows (configs[4] read as 65 536 negatives per query): the negatives' terms are
            # summed over the whole bank weighted by multiplicity (memory_new._crd_core_scan); only the positives are gathered
            idx1, idx2, scan = nb1, nb2, dict(idx=contrast_idx, col0=1, K=K)
        else:
            # column lists: [num_pos KNN rows of that bank] + [the K sampled negatives]  (:80, :117)
            idx1 = torch.cat((nb1, contrast_idx[:, 1:]), 1).contiguous()
            idx2 = torch.cat((nb2, contrast_idx[:, 1:]), 1).contiguous()
            scan = None
        # out_s = out_v1 comes from bank 2 and is weighted by the bank-2 similarities (:226), and vice versa (:227)
        call = CrdCall(NP, K, NP, K, idx1, idx_bank2=idx2, scan=scan, posw_s=(sim2 / sim2.sum(1, keepdim=True)).contiguous(),
                       posw_t=(sim1 / sim1.sum(1, keepdim=True)).contiguous(), per_sample=True)
        return call, dict(nb1=nb1, nb2=nb2, sim1=sim1, sim2=sim2, _ws=ws)

    def center_columns(self, B, D, batch_label, contrast_idx):
        """:81-101 / :118-139 and ContrastLoss (:241-277) for P = num_pos: columns = [the P - 1 centres of the query's class,
        the K + 1 sampled rows (the first is the query's own), the (C - 1)(P - 1) centres of the other classes, classes
        ascending, centres ascending]; the first P are the positives.  ContrastLoss with P > 1 is
        -(sum_p log_D1_p) / P - sum log_D0 (:268 repeats the negatives' sum P times and divides by P): uniform weights 1 / P,
        what the fused kernels compute for posw = None.  P == 2: the class means (ph_crd_class_centers); P > 2: the device
        k-means (ph_crd_kmeans_centers), both banks in one call, from the PRE-update bank like the means.  Under ReplicaSync
        the banks are replicated and the k-means is deterministic - the same bits on every replica - so no exchange is
        needed.  -> the CrdCall."""
        mem = self.contrast
        K, n, dev = mem.K, mem.nLem, contrast_idx.device
        C = len(mem.class_idx)
        mem.ensure_center_rows(dev)
        P, ck = self.num_pos, self.num_pos - 1
        if ck == 1:
            for bank in (mem.memory_v1, mem.memory_v2):
                check(lib().ph_crd_class_centers(ptr(bank), ptr(mem._members), ptr(mem._member_off), C, mem._max_class, n,
                                                 D, ptr(mem._center_ws), stream()), "ph_crd_class_centers")
        else:
            check(lib().ph_crd_kmeans_centers(ptr(mem.memory_v1), ptr(mem.memory_v2), ptr(mem._members), ptr(mem._member_off),
                                              C, mem._max_class, n, D, ck, self.kmeans_iters, None, None,
                                              ptr(mem._kmeans_ws), stream()), "ph_crd_kmeans_centers")
        # the other classes in ascending order (np.argwhere(onehot == 0)[:, 1], :63-64)
        others = mem._others[batch_label]                                          # [B, C - 1]
        if ck == 1:
            cols = torch.cat(((n + batch_label).view(B, 1), contrast_idx, n + others), 1).contiguous()
        else:
            j = torch.arange(ck, device=dev)
            own = n + batch_label.view(B, 1) * ck + j                              # [B, P - 1]
            neg = (n + others.view(B, C - 1, 1) * ck + j).view(B, (C - 1) * ck)
            cols = torch.cat((own, contrast_idx, neg), 1).contiguous()
        Kn = K + (C - 1) * ck
        return CrdCall(P, Kn, P, Kn, cols, per_sample=True)                       # (no weights - ContrastLoss: 1 / P each)


def _weighted(sample_weights, rows, mem, B):
    """`rows` [B] = (s + t) sample losses / bsz under the trainer's sample weights -> (loss, the reference's per-sample values)."""
    w = sample_weights.to(rows.device).reshape(-1) if torch.is_tensor(sample_weights) else float(sample_weights)
    bn = float(mem.batch_norm_size or B)                                     # global batch under data parallelism
    sample_loss = w * rows * bn
    return sample_loss.sum(0) / bn, sample_loss


class ContrastLoss_v2(nn.Module):
    """API placeholder: CRD_criterion_v10.py:281-314 is fused into ph_crd_loss_grad (similarity-weighted positives)."""

    def __init__(self, n_data):
        super().__init__()
        self.n_data = n_data

    def forward(self, *a, **k):
        raise NotImplementedError("fused into the CRD loss kernel; call CRDLoss.forward")
