"""What train() of the three stage-2 trainers keeps between the batch body and the test pass, on the device (DESIGN.md
section 30; csrc/epochrec.hip): the epoch bookkeeping as one launch at the end of every step - eager or inside the captured
graph - and one device-to-host copy per epoch (`EpochRecord`), the MIA-2023 per-sample stores (`FeatureStores`) and the
similarity audit over them (`sim_audit`, behind evaluate.feature_audit_device / logit_audit_device).  The stage-1
trainers' counterpart is `Stage1Record` at the end of this file.

The reference reads every one of these values on the host each step (MICCAI-2022 train_test_path_multi_distill.py:305,
:317-324, :340; "MIA 2023/stage2_unimodal_student/train_test_path_multi_distill.py":338-342, :380-383, :423, :435-442, :459)."""
import ctypes as C

import numpy as np
import torch

from ._lib import check, lib, ptr, require_cuda, stream

REC_WORDS = 56                      # PH_EPOCHREC_WORDS
REC_ADD, REC_ADD_POSITIVE = 0, 1    # PH_REC_ADD, PH_REC_ADD_POSITIVE
AUDIT_MAX_N, AUDIT_MAX_D = 65536, 512


def _f32c(t, name):
    require_cuda(t, name)
    if t.dtype != torch.float32 or not t.is_contiguous():
        raise ValueError("%s: a contiguous float32 device tensor (got %s)" % (name, t.dtype))
    return t


def record_add(buf, scalars=(), modes=(), wvec=None, pred=None, grade=None, rows=()):
    """ph_epoch_record_add on the current stream: `scalars` one-element float32 device tensors with their `modes`, `wvec` a
    float32 vector of up to 16 entries, (`pred` [B, C], `grade` int64 [B]) for the correct count, `rows` up to two float32
    vectors of one length whose means are added.  A refused argument is a ValueError; nothing is launched then."""
    ns = len(scalars)
    if ns != len(modes) or ns > 16 or len(rows) > 2:
        raise ValueError("record_add: up to 16 scalars with one mode each, up to two rows")
    for t in scalars:
        if _f32c(t, "scalar").numel() != 1:
            raise ValueError("record_add: every scalar is a one-element tensor")
    sp = (C.c_void_p * max(ns, 1))(*[t.data_ptr() for t in scalars])
    md = (C.c_int32 * max(ns, 1))(*[int(m_) for m_ in modes])
    B = Cc = 0
    if pred is not None:
        _f32c(pred, "pred")
        if pred.dim() != 2 or grade is None or grade.dtype != torch.int64 or grade.numel() != pred.shape[0] \
                or not grade.is_contiguous():
            raise ValueError("record_add: pred [B, C] float32 with grade int64 [B]")
        require_cuda(grade, "grade")
        B, Cc = pred.shape
    rows = [_f32c(r, "row").reshape(-1) for r in rows]
    if len(rows) == 2 and rows[0].numel() != rows[1].numel():
        raise ValueError("record_add: both rows have one length")
    nw = 0 if wvec is None else _f32c(wvec, "wvec").numel()
    rc = lib().ph_epoch_record_add(ptr(buf), C.cast(sp, C.c_void_p) if ns else None, C.cast(md, C.c_void_p) if ns else None, ns,
                                   ptr(wvec), nw, ptr(pred), ptr(grade) if pred is not None else None, B, Cc,
                                   ptr(rows[0]) if rows else None, ptr(rows[1]) if len(rows) == 2 else None,
                                   rows[0].numel() if rows else 0, stream())
    if rc == -22:
        raise ValueError("record_add: at most 16 scalars / weights, 1 <= B <= 1048576, 1 <= C <= 16, rows of 1 .. 1048576 "
                         "entries, and something to add")
    check(rc, "ph_epoch_record_add")


def store_rows(store, index, rows, skipped, softmax=False):
    """store[index] = rows (softmax(rows, 1) first with `softmax`), ph_store_rows: the last of equal indices wins, an index
    outside the store is skipped and counted in `skipped` (int64 [1], device)."""
    _f32c(store, "store"); _f32c(rows, "rows")
    if rows.dim() != 2 or store.dim() != 2 or store.shape[1] != rows.shape[1] or index.dtype != torch.int64 \
            or index.numel() != rows.shape[0] or not index.is_contiguous() or skipped.dtype != torch.int64:
        raise ValueError("store_rows: store [n, D], rows [B, D] float32, index int64 [B], skipped int64 [1]")
    require_cuda(index, "index"); require_cuda(skipped, "skipped")
    rc = lib().ph_store_rows(ptr(rows), ptr(index), rows.shape[0], rows.shape[1], ptr(store), store.shape[0], int(bool(softmax)),
                             ptr(skipped), stream())
    if rc == -22:
        raise ValueError("store_rows: 1 <= B <= 65536, 1 <= D <= 4096, 1 <= n (got B %d, D %d, n %d)"
                         % (rows.shape[0], rows.shape[1], store.shape[0]))
    check(rc, "ph_store_rows")


def sim_audit(fuse, path, labels=None):
    """ph_sim_audit -> one int64 [8] device tensor: words 0-4 the float64 sums (teacher intra, teacher inter, student intra,
    student inter, sum |S_f - S_p|), words 5-6 the intra / inter pair counts.  No host read."""
    _f32c(fuse, "fuse"); _f32c(path, "path")
    if fuse.dim() != 2 or path.dim() != 2 or fuse.shape[0] != path.shape[0]:
        raise ValueError("sim_audit: two stores [n, Df] and [n, Dp] over the same rows")
    n, Df, Dp = fuse.shape[0], fuse.shape[1], path.shape[1]
    nbytes = lib().ph_sim_audit_workspace_bytes(n, Df, Dp) if max(n, Df, Dp) < 2 ** 31 else 0
    if nbytes == 0:
        raise ValueError("sim_audit: 1 <= n <= %d rows and 1 <= D <= %d columns (got n %d, D %d and %d)"
                         % (AUDIT_MAX_N, AUDIT_MAX_D, n, Df, Dp))
    if labels is not None:
        require_cuda(labels, "labels")
        if labels.numel() != n:
            raise ValueError("sim_audit: one label per row")
        labels = labels.reshape(-1).to(torch.int64).contiguous()
    out = torch.empty(8, device=fuse.device, dtype=torch.int64)
    ws = torch.empty(nbytes, device=fuse.device, dtype=torch.uint8)
    check(lib().ph_sim_audit(ptr(fuse), ptr(path), ptr(labels), n, Df, Dp, out.data_ptr(), out.data_ptr() + 40, ptr(ws),
                             stream()), "ph_sim_audit")
    return out


def audit_means(words):
    """The one host read of an audit: the int64 [8] tensor of `sim_audit` -> the reference's five means (numpy float64; a class
    split without inter-class pairs gives NaN there, as numpy's mean of an empty selection)."""
    w = words.cpu().numpy()
    s, c = w[:5].view(np.float64), w[5:7]
    with np.errstate(invalid="ignore", divide="ignore"):
        intra, inter, n2 = np.float64(c[0]), np.float64(c[1]), np.float64(c[0] + c[1])
        return dict(teacher_intra=s[0] / intra, teacher_inter=s[1] / inter, student_intra=s[2] / intra,
                    student_inter=s[3] / inter, similarity_diff=s[4] / n2, intra_pairs=int(c[0]), inter_pairs=int(c[1]))


class EpochRecord:
    """The epoch sums of a DistillStep on the device.  `step.record = EpochRecord(step)` makes every step - eager or replayed
    from the captured graph - end with one ph_epoch_record_add; `reset()` is a memset on the stream at epoch start, `read()`
    the one device-to-host copy of the epoch.  Attach it before the graph is captured (before the third step)."""

    def __init__(self, step):
        if step.sync is not None:
            raise NotImplementedError("EpochRecord under data parallelism (the replicas' records are not summed)")
        self.variant = step.variant
        self.gk = step.plan.weighting == "gk"          # `loss_weights += scale` runs only under --assign_weights True
        self.beta = float(step.opt.beta)
        self.buf = torch.zeros(REC_WORDS, device=step.device, dtype=torch.int64)
        self.n_weights = 0

    def reset(self):
        self.buf.zero_()

    def add(self, out, loss_div, loss_kd, grade):
        """The end of a step: `out` the step's result, `loss_div` the unscaled KL sum (:266 / :268 / :270), `loss_kd`
        opt.beta * (kd1 + kd2) (:315) - one-element device tensors the step formed itself."""
        scale = out["scale"] if self.gk else None
        if scale is not None:
            scale = scale.reshape(-1).contiguous()
            self.n_weights = scale.numel()
        rows = [out[k].reshape(-1) for k in ("w1", "w2") if self.variant == "mia2023" and k in out]
        if grade.dtype != torch.int64:
            grade = grade.long()
        record_add(self.buf, (out["loss"].reshape(1), out["loss_cls"].reshape(1), loss_div.reshape(1), loss_kd.reshape(1)),
                   (REC_ADD, REC_ADD, REC_ADD_POSITIVE, REC_ADD_POSITIVE), scale, out["pred_path"], grade, rows)

    def read(self):
        w = self.buf.cpu().numpy()
        f = w.view(np.float64)
        steps = int(w[36])
        d = dict(loss_epoch=float(f[0]), loss_cls_epoch=float(f[1]), loss_div_epoch=float(f[2]), loss_kd_epoch=float(f[3]),
                 loss_weights=f[16:16 + self.n_weights].copy() if self.gk else None, grad_path_epoch=int(w[34]),
                 bad_labels=int(w[35]), rows=int(w[37]), steps=steps, loss_div_added=int(w[42]), loss_kd_added=int(w[43]))
        if self.variant == "mia2023":
            # np.mean of the per-step means (:475-476)
            d["teacher1_query_weight"] = float(f[32]) / steps if steps else float("nan")
            d["teacher2_query_weight"] = float(f[33]) / steps if steps else float("nan")
        return d


class FeatureStores:
    """The four [n_data, .] stores of the MIA-2023 trainer (:300-304, :338-342) on the device, filled inside the step:
    `step.stores = FeatureStores(step, n_data)`.  fuse_feat / path_feat: the teacher's and the student's feature rows;
    fuse_pred / path_pred: softmax of logits[-1] and of logit_path.  Allocated at the first step (the widths are the
    networks')."""
    NAMES = ("fuse_feat", "path_feat", "fuse_pred", "path_pred")

    def __init__(self, step, n_data):
        if step.variant != "mia2023":
            raise ValueError("FeatureStores belong to variant 'mia2023'")
        if step.sync is not None:
            raise NotImplementedError("FeatureStores under data parallelism")
        if n_data < 1:
            raise ValueError("n_data >= 1")
        self.n_data, self.device = int(n_data), step.device
        self.skipped = torch.zeros(1, device=step.device, dtype=torch.int64)
        self.fuse_feat = self.path_feat = self.fuse_pred = self.path_pred = None

    def add(self, out, index):
        if index.dtype != torch.int64:
            index = index.long()
        srcs = (out["fuse_feat"], out["path_feat"], out["fuse_logit"], out["logit_path"])
        for name, src, sm in zip(self.NAMES, srcs, (False, False, True, True)):
            src = src.detach()
            if src.dtype != torch.float32 or not src.is_contiguous():
                src = src.float().contiguous()
            if getattr(self, name) is None:
                setattr(self, name, torch.zeros(self.n_data, src.shape[1], device=self.device, dtype=torch.float32))
            store_rows(getattr(self, name), index, src, self.skipped, softmax=sm)


# ------------------------------------------------------------------------------------------------ stage 1
S1_WORDS = 48                       # PH_STAGE1REC_WORDS
S1_MAX_B, S1_MAX_CAP = 65536, 1 << 20
S1_COLUMNS = ("h_fuse", "h_path", "h_omic", "censor", "survtime")


def stage1_record_add(buf, scalars=(), modes=(), heads=(), grade=None, cols=None, store=None):
    """ph_stage1_record_add on the current stream: `scalars` / `modes` as in record_add, `heads` up to three float32 [B, C]
    predictions against `grade` int64 [B], `cols` the five float32 [B] survival columns (S1_COLUMNS) appended to `store`
    float32 [5, cap] at the cursor the record keeps.  A refused argument is a ValueError; nothing is launched then."""
    ns = len(scalars)
    if ns != len(modes) or ns > 16 or len(heads) > 3:
        raise ValueError("stage1_record_add: up to 16 scalars with one mode each, up to three heads")
    for t in scalars:
        if _f32c(t, "scalar").numel() != 1:
            raise ValueError("stage1_record_add: every scalar is a one-element tensor")
    sp = (C.c_void_p * max(ns, 1))(*[t.data_ptr() for t in scalars])
    md = (C.c_int32 * max(ns, 1))(*[int(m_) for m_ in modes])
    B = Cc = cap = 0
    if heads:
        B, Cc = heads[0].shape if heads[0].dim() == 2 else (0, 0)
        for h in heads:
            if _f32c(h, "head").dim() != 2 or tuple(h.shape) != (B, Cc):
                raise ValueError("stage1_record_add: every head is float32 [B, C]")
        if grade is None or grade.dtype != torch.int64 or grade.numel() != B or not grade.is_contiguous():
            raise ValueError("stage1_record_add: heads [B, C] float32 with grade int64 [B]")
        require_cuda(grade, "grade")
    elif grade is not None:
        raise ValueError("stage1_record_add: grade without a head")
    if (cols is None) != (store is None):
        raise ValueError("stage1_record_add: the five survival columns and the store, or neither")
    if cols is not None:
        if len(cols) != 5:
            raise ValueError("stage1_record_add: five survival columns %s" % (S1_COLUMNS,))
        cols = [_f32c(c, "column").reshape(-1) for c in cols]
        n = cols[0].numel()
        if any(c.numel() != n for c in cols) or (heads and n != B):
            raise ValueError("stage1_record_add: the survival columns have one length, the heads' B")
        if _f32c(store, "store").dim() != 2 or store.shape[0] != 5:
            raise ValueError("stage1_record_add: store float32 [5, cap]")
        B, cap = n, store.shape[1]
    hp = [ptr(h) for h in heads] + [None] * (3 - len(heads))
    cp = [ptr(c) for c in cols] if cols is not None else [None] * 5
    if max(B, Cc, cap) >= 2 ** 31:
        raise ValueError("stage1_record_add: sizes beyond int32")
    rc = lib().ph_stage1_record_add(ptr(buf), C.cast(sp, C.c_void_p) if ns else None, C.cast(md, C.c_void_p) if ns else None, ns,
                                    hp[0], hp[1], hp[2], len(heads), ptr(grade) if heads else None, B, Cc, cp[0], cp[1], cp[2],
                                    cp[3], cp[4], ptr(store), cap, stream())
    if rc == -22:
        raise ValueError("stage1_record_add: at most 16 scalars and 3 heads, 1 <= B <= %d, 1 <= C <= 16, 1 <= cap <= %d, and "
                         "something to add (got B %d, C %d, cap %d)" % (S1_MAX_B, S1_MAX_CAP, B, Cc, cap))
    check(rc, "ph_stage1_record_add")


class Stage1Record:
    """The epoch sums of a TeacherStage1Step on the device.  `step.record = Stage1Record(step, n_rows)` makes every step - eager,
    masking or replayed from either captured graph - end with one ph_stage1_record_add; `reset()` is a memset on the stream at
    epoch start (it also rewinds the survival store's cursor), `read()` the one device-to-host copy of the epoch.  Attach it
    before the graph is captured (before the third step).  `n_rows`: the rows an epoch offers (the survival store's columns).

    What is added, in the order of "MIA 2022/train_test_tSVD.py":455-467 (MICCAI-2022/train_test_MT.py:224-233 and MIA-2023
    train_test_MT_SP_Masking.py:310-325 agree where they have the term): loss, the fuse / path / omic branch loss (the NLL
    value under grading, the Cox term under survival: the reference's other addend is the Python integer 0), and only when
    > 0.0 loss_tsvd, loss_CRD, loss_pred_KD, loss_pred_KD_masking.  On a step that ran the t-SVD auxiliary update the two
    nuclear norms follow (:392, :409 - `avg_path_TNN += path_TNN` without a test, under conditions that are always true (:379,
    :400), so both are added whatever tSVD_mode is; update_aux's source is absent from the reference, its TNN is a float32
    device scalar here and is widened like every other scalar)."""
    SCALARS = ("loss", "loss_fuse", "loss_path", "loss_omic", "loss_tsvd", "loss_CRD", "loss_KD", "loss_pred_KD_masking",
               "avg_path_TNN", "avg_omic_TNN")
    MODES = (REC_ADD,) * 4 + (REC_ADD_POSITIVE,) * 4 + (REC_ADD,) * 2

    def __init__(self, step, n_rows):
        if step.sync is not None:
            raise NotImplementedError("Stage1Record under data parallelism (the replicas' records are not summed)")
        self.surv = bool(step.surv)
        self.n_rows = int(n_rows)
        if self.surv and not 1 <= self.n_rows <= S1_MAX_CAP:
            raise ValueError("Stage1Record: 1 <= n_rows <= %d (the range of ph_cindex_counts), got %d" % (S1_MAX_CAP, self.n_rows))
        self.buf = torch.zeros(S1_WORDS, device=step.device, dtype=torch.int64)
        self.store = torch.zeros(5, self.n_rows, device=step.device, dtype=torch.float32) if self.surv else None
        self.rows_host = 0

    def reset(self):
        self.buf.zero_()
        self.rows_host = 0

    def count_rows(self, n):
        self.rows_host += int(n)

    def add(self, out, grade, tnns=None, survtime=None, censor=None):
        """The end of a step: `out` the step's result, `tnns` (path_TNN, omic_TNN) on a step that ran the auxiliary update."""
        branch = ("loss_cox_fuse", "loss_cox_path", "loss_cox_omic") if self.surv else ("loss_nll_fuse", "loss_nll_path",
                                                                                        "loss_nll_omic")
        sc = [out[k] for k in ("loss",) + branch + ("loss_tsvd", "loss_CRD", "loss_pred_KD", "loss_pred_KD_masking")]
        if tnns is not None:
            sc += list(tnns)
        sc = [t.reshape(1) for t in sc]
        if self.surv:
            cols = [out["pred"], out["pred_path"], out["pred_omic"], censor, survtime]
            stage1_record_add(self.buf, sc, self.MODES[:len(sc)], cols=cols, store=self.store)
        else:
            if grade.dtype != torch.int64:
                grade = grade.long()
            stage1_record_add(self.buf, sc, self.MODES[:len(sc)], heads=(out["pred"], out["pred_path"], out["pred_omic"]),
                              grade=grade)

    def read(self):
        w = self.buf.cpu().numpy()
        f = w.view(np.float64)
        if int(w[39]):
            raise RuntimeError("Stage1Record: %d survival rows did not fit the store of %d columns" % (int(w[39]), self.n_rows))
        d = {name + "_epoch" if name.startswith("loss") else name: float(f[k]) for k, name in enumerate(self.SCALARS)}
        d.update({name + "_added": int(w[16 + k]) for k, name in enumerate(self.SCALARS)})
        d.update(grad_acc_epoch=int(w[32]), grad_path_epoch=int(w[33]), grad_omic_epoch=int(w[34]), bad_labels=int(w[35]),
                 steps=int(w[36]), rows=int(w[37]), stored=int(w[38]), overflow=int(w[39]))
        return d

    def cindex(self):
        """The epoch's three C-indices (fuse, path, omic; CIndex_lifeline, :523-525) from the device store: one
        ph_cindex_counts launch over its first `rows_host` columns - the host's own count of the batch sizes."""
        from . import ops, utils
        if not self.surv:
            raise ValueError("Stage1Record.cindex belongs to the survival task")
        n = self.rows_host
        if not 2 <= n <= min(self.n_rows, S1_MAX_CAP):
            raise ValueError("Stage1Record.cindex: 2 <= rows <= %d (the store's columns; the range of ph_cindex_counts), got %d"
                             % (min(self.n_rows, S1_MAX_CAP), n))
        col = [self.store[k, :n] for k in range(5)]
        counts = ops.cindex_counts(col[4], col[3], col[:3]).cpu().numpy()
        return tuple(utils.cindex_from_counts(c) for c in counts)
