"""The input pipeline of the MIA-2023 masking trainer on the device: four augmented views with superpixel label maps
(augment.DeviceAugmentSP), the resident loader that emits the trainer's batch tuple (augment.ResidentSuperpixelLoader),
and TeacherStage1Step fed by it."""
import itertools
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _src(B, SH, SW, seed):
    g = torch.Generator().manual_seed(seed)
    base = torch.randint(0, 256, (B, SH // 8, SW // 8, 3), generator=g, dtype=torch.uint8)
    img = base.repeat_interleave(8, 1).repeat_interleave(8, 2).int() + torch.randint(-20, 21, (B, SH, SW, 3), generator=g)
    return img.clamp(0, 255).to(torch.uint8)


def _opt(S, **kw):
    return types.SimpleNamespace(input_size_path=S, **kw)


def _flip_crop(a, p, S):
    if p[0]:
        a = a[:, ::-1]
    if p[1]:
        a = a[::-1]
    return a[int(p[2]):int(p[2]) + S, int(p[3]):int(p[3]) + S]


def test_four_views_and_label_maps_equal_oracle_for_given_draws():
    """All 24 step orders, both flips, corner crops: every float view equals oracle.augment.one_view bit for bit; the two
    label maps equal the numpy flip + crop of the int16 map under view 0's / view 1's parameters."""
    import multimodal_learning_amd as m
    from oracle import augment as OA
    B, SH, SW, S, V = 12, 96, 80, 64, 4
    src = _src(B, SH, SW, 1)
    sp = torch.randint(0, 300, (B, SH, SW), generator=torch.Generator().manual_seed(2)).to(torch.int16)
    orders = list(itertools.permutations(range(4)))
    rng = np.random.default_rng(0)
    prm = torch.zeros(B, V, 16)
    dicts = {}
    for b in range(B):
        for v in range(V):
            k = b * V + v
            d = dict(flipH=int(k & 1), flipV=int((k >> 1) & 1), top=int([0, SH - S, rng.integers(0, SH - S + 1)][k % 3]),
                     left=int([SW - S, 0, rng.integers(0, SW - S + 1)][k % 3]), S=S, b=float(np.float32(rng.uniform(0.9, 1.1))),
                     c=float(np.float32(rng.uniform(0.9, 1.1))), s=float(np.float32(rng.uniform(0.95, 1.05))),
                     h=float(np.float32(rng.uniform(-0.01, 0.01))), order=orders[k % 24])
            dicts[(b, v)] = d
            prm[b, v, :12] = torch.tensor([d["flipH"], d["flipV"], d["top"], d["left"], d["b"], d["c"], d["s"], d["h"], *d["order"]])
    aug = m.augment.DeviceAugmentSP(_opt(S))
    x0, l0, x1, l1, x2, x3 = aug(src.cuda(), sp.cuda(), params=prm)
    outs = [t.cpu().numpy() for t in (x0, x1, x2, x3)]
    worst = 0.0
    for (b, v), d in dicts.items():
        ref, mean = OA.one_view(src[b].numpy(), d)
        assert int(aug.last_params[b, v, 12]) == mean, (b, v)
        worst = max(worst, float(np.abs(outs[v][b] - ref).max()))
    assert worst == 0.0, worst
    assert l0.dtype == torch.int64 and tuple(l0.shape) == (B, S, S) and l1.dtype == torch.int64
    for b in range(B):
        for v, l in enumerate((l0, l1)):
            want = _flip_crop(sp[b].numpy(), prm[b, v].numpy(), S)
            assert np.array_equal(l[b].cpu().numpy(), want.astype(np.int64)), (b, v)


def test_views_0_and_1_are_the_two_view_augmenter_bit_for_bit():
    """Same seed and step counter: views 0, 1 and their parameter rows are DeviceAugment's; views 2, 3 are other draws."""
    import multimodal_learning_amd as m
    B, SH, SW, S = 32, 72, 96, 56
    src = _src(B, SH, SW, 11).cuda()
    sp = torch.zeros(B, SH, SW, dtype=torch.int16, device="cuda")
    a2 = m.augment.DeviceAugment(_opt(S), seed=5)
    a4 = m.augment.DeviceAugmentSP(_opt(S), seed=5)
    for step in range(3):
        y0, y1 = a2(src)
        x0, _, x1, _, x2, x3 = a4(src, sp)
        p2, p4 = a2.last_params.cpu(), a4.last_params.cpu()
        assert tuple(p4.shape) == (B, 4, 16) and torch.equal(p4[:, :2], p2), step
        assert torch.equal(x0, y0) and torch.equal(x1, y1), step
        for a, b in itertools.combinations(range(4), 2):
            assert not torch.equal(p4[:, a, :12], p4[:, b, :12]), (step, a, b)
        assert not torch.equal(x2, x0) and not torch.equal(x2, x1) and not torch.equal(x3, x0) and not torch.equal(x3, x1)
        assert not torch.equal(x2, x3)
        p = p4[:, 2:].reshape(-1, 16).numpy()
        assert set(np.unique(p[:, 0])) <= {0.0, 1.0} and p[:, 2].min() >= 0 and p[:, 2].max() <= SH - S and p[:, 3].max() <= SW - S
        assert all(sorted(o) == [0, 1, 2, 3] for o in p[:, 8:12].astype(int).tolist())
    # with a row gather straight from a store
    rows = torch.tensor([3, 3, 0, 31, 7], device="cuda")
    b2 = m.augment.DeviceAugment(_opt(S), seed=9); b4 = m.augment.DeviceAugmentSP(_opt(S), seed=9)
    y0, y1 = b2(src, rows=rows)
    x0, _, x1, _, _, _ = b4(src, sp, rows=rows)
    assert torch.equal(x0, y0) and torch.equal(x1, y1)


def _loader(n=24, SH=96, S=64, K=30, seed=3, n_rows=None, **kw):
    import multimodal_learning_amd as m
    tiles = _src(n, SH, SH, 5).cuda()
    n_rows = n_rows or n
    labels = torch.arange(n_rows) % 3
    opt = _opt(S, nce_p=4, nce_k=10, pos_mode="multi_pos", label_dim=3, num_superpixels=K, **kw)
    ld = m.augment.ResidentSuperpixelLoader(opt, tiles, torch.randn(n_rows, 80), labels, seed=seed)
    return m, ld, opt, tiles, labels


def test_resident_superpixel_loader_tuple_and_in_place_refill():
    m, ld, opt, tiles, labels = _loader()
    n, SH, S = 24, 96, 64
    N = m.superpixel.slic_num_labels(SH, SH, 30)
    maps, _ = m.superpixel.slic_segment(tiles, 30)
    assert ld.num_labels == N == opt.num_superpixels_max and torch.equal(ld.sp_maps, maps) and ld.sp_maps.dtype == torch.int16
    idx = torch.tensor([7, 0, 23, 12, 12, 19])
    bt = ld.batch(idx)
    (xp, spm, exp_, espm, m1, m2), z0, xo, z1, z2, gr, index, sidx = bt
    for t in (xp, exp_, m1, m2):
        assert t.dtype == torch.float32 and tuple(t.shape) == (6, 3, S, S)
    for t in (spm, espm):
        assert t.dtype == torch.int64 and tuple(t.shape) == (6, S, S) and int(t.min()) >= 0 and int(t.max()) < N
    assert tuple(xo.shape) == (6, 80) and torch.equal(gr.cpu(), labels[idx]) and torch.equal(index.cpu(), idx)
    assert tuple(sidx.shape) == (6, 4 + 10) and torch.equal(sidx[:, 0].cpu(), idx) and float(z0.abs().sum()) == 0.0
    prm = ld.aug.last_params.cpu().numpy()
    for b in range(6):
        for v, l in enumerate((spm, espm)):
            assert np.array_equal(l[b].cpu().numpy(), _flip_crop(maps[idx[b]].cpu().numpy(), prm[b, v], S).astype(np.int64))
    # the float views are DeviceAugmentSP's on the gathered tiles with the same draws
    ref = m.augment.DeviceAugmentSP(opt)(tiles[idx.cuda()], maps[idx.cuda()], params=ld.aug.last_params.clone())
    for got, want in zip(bt[0], ref):
        assert torch.equal(got, want)
    # refill in place
    flat = list(bt[0]) + [bt[2], bt[5], bt[6], bt[7]]
    ptrs = [t.data_ptr() for t in flat]
    old = bt[0][0].clone()
    idx2 = torch.tensor([2, 6, 10, 23, 1, 1])
    bt2 = ld.batch(idx2, into=bt)
    assert [t.data_ptr() for t in list(bt2[0]) + [bt2[2], bt2[5], bt2[6], bt2[7]]] == ptrs
    ref = m.augment.DeviceAugmentSP(opt)(tiles[idx2.cuda()], maps[idx2.cuda()], params=ld.aug.last_params.clone())
    for got, want in zip(bt2[0], ref):
        assert torch.equal(got, want)
    assert not torch.equal(bt2[0][0], old) and torch.equal(bt2[6].cpu(), idx2) and torch.equal(bt2[5].cpu(), labels[idx2])
    assert torch.equal(bt2[2].cpu(), ld.x_omic[idx2.cuda()].cpu()) and torch.equal(bt2[7][:, 0].cpu(), idx2)
    # next(): endless shuffled run, also in place
    bt3 = ld.next(into=bt2)
    assert [t.data_ptr() for t in list(bt3[0]) + [bt3[2], bt3[5], bt3[6], bt3[7]]] == ptrs and int(ld.batch_no.item()) == 1
    bt4 = ld.next(batch_size=8)
    assert tuple(bt4[0][1].shape) == (8, S, S) and len(bt4[0]) == 6


def test_loader_keeps_a_given_num_superpixels_max_and_shares_maps_between_rows():
    m, ld, opt, tiles, labels = _loader(n=8, n_rows=24, num_superpixels_max=77)
    assert opt.num_superpixels_max == 77 and ld.num_labels == m.superpixel.slic_num_labels(96, 96, 30)
    ld.row_to_tile = torch.arange(24, device="cuda") % 8
    S = 64
    idx = torch.tensor([1, 9, 17, 2])                       # rows 1, 9, 17 share tile 1
    (xp, spm, _, espm, _, _), *_ = ld.batch(idx)
    prm = ld.aug.last_params.cpu().numpy()
    for b, tile in enumerate((1, 1, 1, 2)):
        for v, l in enumerate((spm, espm)):
            want = _flip_crop(ld.sp_maps[tile].cpu().numpy(), prm[b, v], S)
            assert np.array_equal(l[b].cpu().numpy(), want.astype(np.int64)), (b, v)


def test_stage1_masking_step_fed_by_the_resident_superpixel_loader(monkeypatch):
    """The shipped command (--masking 1 --Path_K 1 --Omic_K 5) end to end: batches from the loader at epoch 2 for three
    steps.  Relation and tolerance of tests/test_gpu_step.py::test_stage1_step_with_superpixel_masking_terms: on the
    first batch (the weights of the two steps are still equal) loss = loss of the same step without the term + the term;
    at epoch 1 the term is 0.  The attention mask call gets N from opt.num_superpixels_max: no sp_mask.max() read-back."""
    import multimodal_learning_amd as m
    from oracle import weights as W
    B, S, SH, n = 4, 64, 96, 24
    m.set_precision("bf16x6")
    try:
        def build():
            opt = m.stage2_opt(dropout_rate=0.0, batch_size=B, cut_fuse_grad=False, num_teachers=2)
            opt.pred_distill, opt.KD_weight, opt.CRD_distill, opt.SP_distill, opt.orth_loss = 1, 1.0, 0, 0, "False"
            opt.masking, opt.start_epoch, opt.Path_K, opt.Omic_K = 1, 1, 1, 5
            opt.input_size_path, opt.nce_p, opt.nce_k, opt.pos_mode, opt.num_superpixels = S, 4, 10, "multi_pos", 30
            model = m.define_net(opt, 1); ema = m.define_net(opt, 1)
            model.load_state_dict(W.make_state_dict(W.teacher_shapes(320), 3)); ema.load_state_dict(W.make_state_dict(W.teacher_shapes(320), 4))
            return m.TeacherStage1Step(opt, device="cuda", models=(model.cuda(), ema.cuda())), opt
        st, opt = build()
        st0, opt0 = build()
        tiles = _src(n, SH, SH, 8).cuda()
        g = torch.Generator().manual_seed(1)
        ld = m.augment.ResidentSuperpixelLoader(opt, tiles, torch.randn(n, 320, generator=g), torch.arange(n) % 3, seed=2)
        N = ld.num_labels
        assert opt.num_superpixels_max == N
        opt0.num_superpixels_max = N
        seen = []
        real = m.superpixel.superpixel_topk_mask

        def spy(x_path_grad, sp_mask, path_k, num_superpixels=None, return_mean=False):
            seen.append(num_superpixels)
            return real(x_path_grad, sp_mask, path_k, num_superpixels, return_mean)
        monkeypatch.setattr(m.superpixel, "superpixel_topk_mask", spy)
        bt = ld.next(batch_size=B)
        assert len(bt[0]) == 6
        out0 = st0.step(bt, epoch=1)                      # epoch <= start_epoch: term off
        assert float(out0["loss_pred_KD_masking"]) == 0.0 and seen == []
        out = st.step(bt, epoch=2)
        term = float(out["loss_pred_KD_masking"])
        print("loss %.6f  without the term %.6f  term %.6f" % (float(out["loss"]), float(out0["loss"]), term))
        assert torch.isfinite(out["loss"]) and term > 0
        assert abs(float(out["loss"]) - float(out0["loss"]) - term) <= 1e-3 * abs(float(out["loss"]))
        for _ in range(2):
            bt = ld.next(into=bt)
            out = st.step(bt, epoch=2)
            assert all(torch.isfinite(out[k]) for k in ("loss", "loss_nll", "loss_pred_KD", "loss_pred_KD_masking"))
            assert float(out["loss_pred_KD_masking"]) > 0
        assert seen == [N, N, N]
        assert torch.isfinite(st.optimizer.flat.grad).all()
    finally:
        m.set_precision("bf16")
