"""On-device input pipeline: the training transform of the reference's loader
(MICCAI-2022/data_loaders_MT.py:168-175 run twice by `TransformTwice`, :51-53) on uint8 source tiles that stay resident in
HBM - at the step rates of this package the PIL pipeline in four DataLoader workers is the bottleneck.

    aug = DeviceAugment(opt, device)                    # opt.input_size_path = crop size
    x_path, ema_x_path = aug(src_u8)                    # src_u8 [B, SH, SW, 3] uint8 (device) -> two f32 [B, 3, S, S] views

`DeviceAugmentSP` / `ResidentSuperpixelLoader`: the four views and superpixel label maps of the MIA-2023 masking loader.

The draws come from a counter RNG keyed by (seed, step, image, view) - reproducible, not numpy's stream.  The colour
arithmetic is Pillow's as torchvision drives it, pinned bit for bit against Pillow (tests/golden/colorjitter_pil.npz)."""
import torch

from ._lib import lib, check, ptr, stream, require_cuda

NPARAM = 16


class DeviceAugment:
    def __init__(self, opt, device="cuda", seed=0, brightness=0.1, contrast=0.1, saturation=0.05, hue=0.01):
        self.S = int(opt.input_size_path)
        self.device = torch.device(device)
        self.seed = int(seed)
        self.jitter = (float(brightness), float(contrast), float(saturation), float(hue))     # :172
        self.step = torch.zeros(1, device=self.device, dtype=torch.int64)                      # device-side draw counter
        self.last_params = None

    def __call__(self, src_u8, params=None, rows=None, out=None):
        """`rows` (int64 [B], device): take the batch straight out of a resident tile store src_u8 [n, SH, SW, 3] - no
        gather copy of the 3 MB source tiles."""
        src = require_cuda(src_u8, "src_u8")
        if src.dtype != torch.uint8 or src.dim() != 4 or src.shape[3] != 3:
            raise RuntimeError("src_u8 must be uint8 [B, SH, SW, 3]")
        src = src.contiguous()
        _, SH, SW, _ = src.shape
        if rows is not None:
            rows = rows.to(src.device).long().contiguous()
        B = src.shape[0] if rows is None else rows.shape[0]
        S = self.S
        if params is None:
            params = torch.empty(B, 2, NPARAM, device=src.device, dtype=torch.float32)
            check(lib().ph_augment_params(ptr(params), B, self.seed, ptr(self.step), SH, SW, S, *self.jitter, stream()),
                  "ph_augment_params")
            self.step += 1
        else:
            # Caller-supplied parameters (tests, replaying a recorded draw; not the hot path, so a host check is fine).
            # Layout [B, 2, NPARAM]: 0-11 flips / crop / jitter factors / step order (oracle/augment.py::draw_params),
            # 12 and 14-15 scratch (zeroed here), 13 = BIT MASK of disabled colour steps (bit k set: ColorJitter dropped
            # step k because its range is zero) - the kernel casts it to int, so it must be an integer in 0..15.
            params = params.to(src.device).float().contiguous().clone()
            c13 = params[..., 13]
            if not bool(((c13 >= 0) & (c13 <= 15) & (c13 == c13.round())).all().item()):
                raise ValueError("augmentation params column 13 is the mask of disabled colour steps: integers 0..15 "
                                 "(got values outside that set - a parameter block from before the layout change?)")
            params[..., 12] = 0
            params[..., 14:] = 0          # the grey-sum accumulator slot (column 13 = mask of disabled steps, kept)
        if out is not None:          # caller-owned buffers (the resident input sets a captured step graph reads from)
            out0, out1 = out
            for t in (out0, out1):
                if tuple(t.shape) != (B, 3, S, S) or t.dtype != torch.float32 or not t.is_contiguous() or not t.is_cuda:
                    raise RuntimeError("out must be two contiguous f32 [B, 3, S, S] device tensors")
        else:
            out0 = torch.empty(B, 3, S, S, device=src.device, dtype=torch.float32)
            out1 = torch.empty_like(out0)
        check(lib().ph_augment_apply(ptr(src), ptr(rows), ptr(params), ptr(out0), ptr(out1), B, SH, SW, S, stream()),
              "ph_augment_apply")
        self.last_params = params
        return out0, out1


class DeviceAugmentSP(DeviceAugment):
    """The transform of the MIA-2023 masking loader (data_loaders_MT_SP.py:352-388, called four times per tile, :446-450):
    four independently drawn views, the superpixel label map carried through the flip and crop of views 0 and 1.

        aug = DeviceAugmentSP(opt, device, seed)
        x_path, sp_mask, ema_x_path, ema_sp_mask, x_path_m_v1, x_path_m_v2 = aug(src_u8, sp_i16)

    src_u8 [n, SH, SW, 3] uint8 and sp_i16 [n, SH, SW] int16 on the device; views f32 [B, 3, S, S], label maps int64
    [B, S, S].  Views 0 and 1 are `DeviceAugment`'s two views for the same seed and step counter, bit for bit (the same
    draws, the same colour kernels); views 2 and 3 extend the keyed counter RNG.  `ema_sp_mask` is the map under view 1 (the
    reference crops the already cropped map a second time, :447, and nothing reads the result)."""
    VIEWS = 4

    def __call__(self, src_u8, sp_i16, params=None, rows=None, out=None):
        import ctypes as C
        src = require_cuda(src_u8, "src_u8")
        if src.dtype != torch.uint8 or src.dim() != 4 or src.shape[3] != 3:
            raise RuntimeError("src_u8 must be uint8 [B, SH, SW, 3]")
        src = src.contiguous()
        sp = require_cuda(sp_i16, "sp_i16")
        if sp.dtype != torch.int16 or tuple(sp.shape) != tuple(src.shape[:3]):
            raise RuntimeError("sp_i16 must be int16 [B, SH, SW] label maps of the same tiles")
        sp = sp.contiguous()
        _, SH, SW, _ = src.shape
        if rows is not None:
            rows = rows.to(src.device).long().contiguous()
        B = src.shape[0] if rows is None else rows.shape[0]
        S, V = self.S, self.VIEWS
        if params is None:
            params = torch.empty(B, V, NPARAM, device=src.device, dtype=torch.float32)
            check(lib().ph_augment_params_v(ptr(params), B, V, self.seed, ptr(self.step), SH, SW, S, *self.jitter, stream()),
                  "ph_augment_params_v")
            self.step += 1
        else:
            # caller-supplied [B, 4, NPARAM] block, the row layout and the column-13 rule of DeviceAugment
            params = params.to(src.device).float().contiguous().clone()
            if tuple(params.shape) != (B, V, NPARAM):
                raise ValueError("augmentation params must be [B, 4, %d]" % NPARAM)
            c13 = params[..., 13]
            if not bool(((c13 >= 0) & (c13 <= 15) & (c13 == c13.round())).all().item()):
                raise ValueError("augmentation params column 13 is the mask of disabled colour steps: integers 0..15")
            params[..., 12] = 0
            params[..., 14:] = 0
        if out is not None:
            x0, l0, x1, l1, x2, x3 = out
            for t in (x0, x1, x2, x3):
                if tuple(t.shape) != (B, 3, S, S) or t.dtype != torch.float32 or not t.is_contiguous() or not t.is_cuda:
                    raise RuntimeError("out views must be contiguous f32 [B, 3, S, S] device tensors")
            for t in (l0, l1):
                if tuple(t.shape) != (B, S, S) or t.dtype != torch.int64 or not t.is_contiguous() or not t.is_cuda:
                    raise RuntimeError("out label maps must be contiguous int64 [B, S, S] device tensors")
        else:
            x0, x1, x2, x3 = (torch.empty(B, 3, S, S, device=src.device, dtype=torch.float32) for _ in range(4))
            l0, l1 = (torch.empty(B, S, S, device=src.device, dtype=torch.int64) for _ in range(2))
        outs = (C.c_void_p * V)(ptr(x0), ptr(x1), ptr(x2), ptr(x3))
        labs = (C.c_void_p * V)(ptr(l0), ptr(l1), None, None)
        check(lib().ph_augment_apply_v(ptr(src), ptr(sp), ptr(rows), ptr(params), outs, labs, B, V, SH, SW, S, stream()),
              "ph_augment_apply_v")
        self.last_params = params
        return x0, l0, x1, l1, x2, x3


class ResidentTileLoader:
    """The training loader's batch tuple (data_loaders_MT.py:256) produced on the device: uint8 tiles, omic vectors and
    labels live in HBM; a batch of row indices becomes ((x_path, ema_x_path), 0, x_omic, 0, 0, grade, index, sample_idx)
    with both augmented views (DeviceAugment, straight from the store) and the contrast indices (ContrastIndexSampler)."""

    def __init__(self, opt, tiles_u8, x_omic, grade, device="cuda", seed=0):
        from .sampler import ContrastIndexSampler
        self.device = torch.device(device)
        self.tiles = require_cuda(tiles_u8, "tiles_u8").contiguous()
        self.x_omic = x_omic.to(self.device).float().contiguous()
        self.grade = grade.to(self.device).long().contiguous()
        self.aug = DeviceAugment(opt, self.device, seed)
        self.sampler = ContrastIndexSampler(opt, self.grade.cpu().numpy(), self.device, seed=seed)
        self.row_to_tile = None       # optional int64 [n_rows]: dataset row -> tile of the store (several rows per tile)
        self.batch_no = None

    def next(self, batch_size=None, into=None):
        """The next batch of an endless shuffled run (DataLoader(shuffle=True, drop_last=True)): its row indices are
        drawn on the device from a device-side batch counter, so the whole call - index draw, both augmented views,
        gathers, contrast indices - is a fixed launch sequence that a HIP graph can capture and replay."""
        from . import ops
        if into is None:
            B = int(batch_size)
            index = torch.empty(B, device=self.device, dtype=torch.int64)
        else:
            index = into[6]
            B = index.shape[0]
        if getattr(self, "batch_no", None) is None:
            self.batch_no = torch.zeros(1, device=self.device, dtype=torch.int64)
        check(lib().ph_shuffle_indices(ptr(index), self.grade.shape[0], B, self.aug.seed, ptr(self.batch_no), stream()),
              "ph_shuffle_indices")
        ops.counter_inc(self.batch_no)
        return self.batch(index, into=into, _index_in_place=into is not None)

    def batch(self, index, into=None, _index_in_place=False):
        """`into`: a previously returned batch tuple whose tensors are refilled in place (fixed addresses: a captured
        step graph that adopted them replays without any staging copy)."""
        index = index.to(self.device).long().contiguous()
        if into is None:
            rows = index if getattr(self, "row_to_tile", None) is None else self.row_to_tile[index]
            x_path, ema_x_path = self.aug(self.tiles, rows=rows)
            grade = self.grade[index]
            z = torch.zeros(index.shape[0], device=self.device)
            return ((x_path, ema_x_path), z, self.x_omic[index], z, z, grade, index, self.sampler(index, grade))
        (x_path, ema_x_path), _, x_omic, _, _, grade, idx_buf, sample_idx = into
        rows = index if getattr(self, "row_to_tile", None) is None else self.row_to_tile[index]
        self.aug(self.tiles, rows=rows, out=(x_path, ema_x_path))
        torch.index_select(self.x_omic, 0, index, out=x_omic)
        torch.index_select(self.grade, 0, index, out=grade)
        if not _index_in_place:
            idx_buf.copy_(index)
        self.sampler(idx_buf, grade, out=sample_idx)
        return into


class ResidentSuperpixelLoader(ResidentTileLoader):
    """The batch tuple of the MIA-2023 stage-1 masking trainer (data_loaders_MT_SP.py:453) produced on the device:
    ((x_path, sp_mask, ema_x_path, ema_sp_mask, x_path_m_v1, x_path_m_v2), 0, x_omic, 0, 0, grade, index, sample_idx).
    At construction the tile store is segmented once (`superpixel.slic_segment`, opt.num_superpixels components,
    compactness 10, as :303-304; `enforce_connectivity` / `min_size_factor`: its connectivity pass, off by default)
    and the int16 maps stay next to the tiles; a batch is four augmented views with the
    label maps of views 0 and 1 (`DeviceAugmentSP`).  `num_labels` is the number of labels N of a map; where the options
    carry no `num_superpixels_max` it is set to N, so that the step's superpixel_attention_mask call reads nothing back."""

    def __init__(self, opt, tiles_u8, x_omic, grade, device="cuda", seed=0, compactness=10, iters=10, chunk=None,
                 enforce_connectivity=False, min_size_factor=0.25):
        from .superpixel import slic_segment
        super().__init__(opt, tiles_u8, x_omic, grade, device, seed)
        self.aug = DeviceAugmentSP(opt, self.device, seed)
        self.sp_maps, self.num_labels = slic_segment(self.tiles, int(opt.num_superpixels), compactness, iters, chunk=chunk,
                                                     enforce_connectivity=enforce_connectivity, min_size_factor=min_size_factor)
        if getattr(opt, "num_superpixels_max", None) is None:
            opt.num_superpixels_max = self.num_labels

    def batch(self, index, into=None, _index_in_place=False):
        index = index.to(self.device).long().contiguous()
        rows = index if getattr(self, "row_to_tile", None) is None else self.row_to_tile[index]
        if into is None:
            views = self.aug(self.tiles, self.sp_maps, rows=rows)
            grade = self.grade[index]
            z = torch.zeros(index.shape[0], device=self.device)
            return (views, z, self.x_omic[index], z, z, grade, index, self.sampler(index, grade))
        views, _, x_omic, _, _, grade, idx_buf, sample_idx = into
        self.aug(self.tiles, self.sp_maps, rows=rows, out=views)
        torch.index_select(self.x_omic, 0, index, out=x_omic)
        torch.index_select(self.grade, 0, index, out=grade)
        if not _index_in_place:
            idx_buf.copy_(index)
        self.sampler(idx_buf, grade, out=sample_idx)
        return into


def patch_offsets(extent, S, grid):
    """Top (or left) offsets of the `grid` overlapping crops of size S along a side of `extent` pixels: k * (extent - S) /
    (grid - 1), which must be an integer; grid = 1 is the centre crop."""
    extent, S, grid = int(extent), int(S), int(grid)
    if grid < 1:
        raise ValueError("grid must be at least 1")
    if S < 1 or S > extent:
        raise ValueError("patch size %d does not fit a side of %d pixels" % (S, extent))
    if grid == 1:
        return [(extent - S) // 2]
    if (extent - S) % (grid - 1):
        raise ValueError("a grid of %d patches of %d over %d pixels has the non-integer stride %d / %d"
                         % (grid, S, extent, extent - S, grid - 1))
    return [k * ((extent - S) // (grid - 1)) for k in range(grid)]


class _Rows:
    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n


class ResidentPatchLoader:
    """The reference's `test_loader_patches` (MICCAI-2022/data_loaders_MT.py:67-77: nine overlapping 512 x 512 patches of
    every 1024 x 1024 test ROI) produced on the device from a resident uint8 store tiles_u8 [n, SH, SW, 3].

    Row r is ROI r // grid^2, grid cell (gy, gx) = divmod(r % grid^2, grid); its crop of size S = opt.input_size_path sits
    at top = gy * (SH - S) / (grid - 1), left = gx * (SW - S) / (grid - 1) (grid = 1: the centre crop).  Iteration yields the
    test loader's 6-tuple (x_path, 0, x_omic, 0, 0, grade) in row order in batches of opt.batch_size, the last one partial
    (shuffle=False, no drop_last), so evaluate.test / test_model / test_teacher consume it unchanged.

    x_path = (u8 / 255 - 0.5) / 0.5 in float32, cut straight out of the store by ph_augment_apply_v with one view, no flip
    and every colour step disabled.  The reference runs its TRAINING transform - random flips and colour jitter - on the
    test patches too, an artefact of reusing PathomicDatasetLoader; that is deliberately not reproduced: a test pass here
    is deterministic.

    `patient`: one hashable id per ROI (None: every ROI its own patient), mapped at construction to dense ids 0..G-1 in
    order of first appearance; a patient whose ROIs carry different grades raises ValueError.  row_patient (int64 [rows],
    device), patients (the ids, host), patient_grade (int64 [G], device), num_patients; group_offsets / group_order: the
    CSR of the rows per patient that evaluate.aggregate_by_patient hands to ph_group_agg / ph_group_quantile.

    `censor`, `survtime`: one value per ROI, both or neither (the survival task).  When given, the
    6-tuple carries them per row at positions 3 and 4 (float32, device) instead of zeros, patient_censor / patient_survtime
    (float32 [G], device; patient_censor_host / patient_survtime_host: numpy) hold one value per patient, and a patient whose
    ROIs disagree in either raises ValueError.  Without them the loader is what it was."""

    def __init__(self, opt, tiles_u8, x_omic, grade, patient=None, grid=3, device="cuda", censor=None, survtime=None):
        import numpy as np
        from .ops import group_csr
        self.device = torch.device(device)
        self.tiles = require_cuda(tiles_u8, "tiles_u8")
        if self.tiles.dtype != torch.uint8 or self.tiles.dim() != 4 or self.tiles.shape[3] != 3:
            raise RuntimeError("tiles_u8 must be uint8 [n, SH, SW, 3]")
        self.tiles = self.tiles.contiguous()
        n, SH, SW, _ = self.tiles.shape
        self.S, self.grid, self.batch_size = int(opt.input_size_path), int(grid), int(opt.batch_size)
        tops, lefts = patch_offsets(SH, self.S, self.grid), patch_offsets(SW, self.S, self.grid)
        if self.batch_size < 1:
            raise ValueError("opt.batch_size must be positive")
        grade_h = np.asarray(grade.cpu() if torch.is_tensor(grade) else grade).reshape(-1).astype(np.int64)
        if grade_h.shape[0] != n or x_omic.shape[0] != n:
            raise ValueError("one omic row and one grade per ROI")
        ids = list(range(n)) if patient is None else list(patient)
        if len(ids) != n:
            raise ValueError("one patient id per ROI")
        if (censor is None) != (survtime is None):
            raise ValueError("censor and survtime come together: both or neither")
        self.has_survival = censor is not None
        if self.has_survival:
            censor_h, survtime_h = (np.asarray(v.cpu() if torch.is_tensor(v) else v).reshape(-1).astype(np.float32)
                                    for v in (censor, survtime))
            if censor_h.shape[0] != n or survtime_h.shape[0] != n:
                raise ValueError("one censor value and one survival time per ROI")
        dense, self.patients, pgrade, first = {}, [], [], []
        roi_patient = np.empty(n, dtype=np.int64)
        for i, pid in enumerate(ids):
            if pid not in dense:
                dense[pid] = len(self.patients)
                self.patients.append(pid)
                pgrade.append(int(grade_h[i]))
                first.append(i)
            elif pgrade[dense[pid]] != int(grade_h[i]):
                raise ValueError("patient %r has ROIs of different grades (%d and %d)" % (pid, pgrade[dense[pid]], int(grade_h[i])))
            elif self.has_survival:
                j = first[dense[pid]]
                if censor_h[j] != censor_h[i] or survtime_h[j] != survtime_h[i]:
                    raise ValueError("patient %r has ROIs of different survival data ((censor, survtime) = (%g, %g) and (%g, %g))"
                                     % (pid, censor_h[j], survtime_h[j], censor_h[i], survtime_h[i]))
            roi_patient[i] = dense[pid]
        self.num_patients = len(self.patients)
        cells = self.grid * self.grid
        self.n_rows = n * cells
        self.dataset = _Rows(self.n_rows)
        row_roi = np.repeat(np.arange(n, dtype=np.int64), cells)
        row_patient = roi_patient[row_roi]
        # one parameter row per patch (the layout of DeviceAugment): flips 0, top, left, factors of the disabled colour
        # steps, order 0 1 2 3, column 13 = 15 (all four steps off)
        prm = np.zeros((self.n_rows, 1, NPARAM), dtype=np.float32)
        cell = np.arange(self.n_rows) % cells
        prm[:, 0, 2] = np.asarray(tops, dtype=np.float32)[cell // self.grid]
        prm[:, 0, 3] = np.asarray(lefts, dtype=np.float32)[cell % self.grid]
        prm[:, 0, 4:7] = 1.0
        prm[:, 0, 8:12] = (0, 1, 2, 3)
        prm[:, 0, 13] = 15
        self.params = torch.from_numpy(prm).to(self.device)
        self.row_roi = torch.from_numpy(row_roi).to(self.device)
        self.row_patient = torch.from_numpy(row_patient).to(self.device)
        self.patient_grade_host = np.asarray(pgrade, dtype=np.int64)
        self.patient_grade = torch.from_numpy(self.patient_grade_host).to(self.device)
        self.x_omic = x_omic.to(self.device).float().contiguous()
        self.grade = torch.from_numpy(grade_h).to(self.device)
        if self.has_survival:
            self.censor = torch.from_numpy(censor_h).to(self.device)
            self.survtime = torch.from_numpy(survtime_h).to(self.device)
            self.patient_censor_host, self.patient_survtime_host = censor_h[first].copy(), survtime_h[first].copy()
            self.patient_censor = torch.from_numpy(self.patient_censor_host).to(self.device)
            self.patient_survtime = torch.from_numpy(self.patient_survtime_host).to(self.device)
        self.group_offsets_host, order = group_csr(row_patient, self.num_patients)
        self.group_offsets = torch.from_numpy(self.group_offsets_host).to(self.device)
        self.group_order = torch.from_numpy(order).to(self.device)

    def __len__(self):
        return (self.n_rows + self.batch_size - 1) // self.batch_size

    def rows(self, lo, hi):
        """The batch of rows lo .. hi - 1."""
        import ctypes as C
        B, S = hi - lo, self.S
        _, SH, SW, _ = self.tiles.shape
        roi = self.row_roi[lo:hi]
        params = self.params[lo:hi].clone()       # the kernel keeps its grey-sum scratch in the row: a fresh copy per call
        x_path = torch.empty(B, 3, S, S, device=self.device, dtype=torch.float32)
        outs = (C.c_void_p * 1)(ptr(x_path))
        check(lib().ph_augment_apply_v(ptr(self.tiles), None, ptr(roi), ptr(params), outs, None, B, 1, SH, SW, S, stream()),
              "ph_augment_apply_v")
        z = torch.zeros(B, device=self.device)
        if self.has_survival:
            return (x_path, z, self.x_omic[roi], self.censor[roi], self.survtime[roi], self.grade[roi])
        return (x_path, z, self.x_omic[roi], z, z, self.grade[roi])

    def __iter__(self):
        for lo in range(0, self.n_rows, self.batch_size):
            yield self.rows(lo, min(lo + self.batch_size, self.n_rows))
