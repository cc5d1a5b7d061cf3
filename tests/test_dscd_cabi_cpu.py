"""The argument rule of the two DSCD entries of csrc/crd.hip, decided on the host before any launch: a machine without a device
returns PH_EINVAL (-22) only from a check that precedes every HIP call.  Pointers are small non-NULL integers that are never
dereferenced by a refused call."""
PH_EINVAL = -22
X = 64      # a non-NULL pointer value for arguments the check must not look behind


def _lib():
    import multimodal_learning_amd as m
    return m.lib()


def test_select_dscd_argument_rule():
    L = _lib()
    call = lambda ptrs, B, P, K, P2, asc, rw: L.ph_crd_select_dscd(*ptrs, B, P, K, P2, asc, rw, None)
    ok = [X, X, X, None, X, X, X]      # diff, out1, out2, ranks (may be NULL), sel, xs, xt
    for k in (0, 1, 2, 4, 5, 6):       # every pointer but ranks
        ptrs = list(ok)
        ptrs[k] = None
        assert call(ptrs, 2, 8, 16, 4, 1, 1) == PH_EINVAL, k
    for a in ((0, 8, 16, 4, 1, 1), (-3, 8, 16, 4, 1, 1),                       # B < 1
              (2, 0, 16, 1, 1, 1), (2, -1, 16, 1, 1, 1),                       # P < 1
              (2, 8, 0, 4, 1, 1), (2, 8, -5, 4, 1, 1),                         # K < 1
              (2, 8, 16, 0, 1, 1), (2, 8, 16, -1, 1, 1), (2, 8, 16, 9, 1, 1),  # P2 outside 1..P
              (2, 8, 16, 4, 2, 1), (2, 8, 16, 4, -1, 0), (2, 8, 16, 4, 1, 2), (2, 8, 16, 4, 0, -1),   # flags outside {0, 1}
              (1, 20481, 1, 8, 1, 0), (1, 1 << 30, 1, 8, 0, 1)):               # a positive list above 160 KiB of LDS (2 P words)
        assert call(ok, *a) == PH_EINVAL, a
    assert 2 * 20480 * 4 == 160 * 1024


def test_loss_grad_one_argument_rule():
    L = _lib()
    # xt, sel, idx, posw (may be NULL), mem, params | T | lossp, dv | B, PK, P2, K2, feat_dim | n_data, inv_bnorm | workspace, stream
    call = lambda head, T, outs, B, PK, P2, K2, D: L.ph_crd_loss_grad_one(*head, T, *outs, B, PK, P2, K2, D, 257.0, 0.5, None, None)
    head, outs = [X, X, X, None, X, X], [X, X]
    for k in (0, 1, 2, 4, 5):
        h = list(head)
        h[k] = None
        assert call(h, 0.07, outs, 2, 40, 4, 16, 128) == PH_EINVAL, k
    for k in (0, 1):
        o = list(outs)
        o[k] = None
        assert call(head, 0.07, o, 2, 40, 4, 16, 128) == PH_EINVAL, k
    for T in (0.0, -0.07, float("nan")):
        assert call(head, T, outs, 2, 40, 4, 16, 128) == PH_EINVAL, T
    for (B, PK, P2, K2, D) in ((0, 40, 4, 16, 128), (-1, 40, 4, 16, 128), (2, 40, 0, 16, 128), (2, 40, 4, -1, 128), (2, 40, 4, 37, 128),
                               (2, 40, 4, 16, 96), (2, 40, 4, 16, 512)):
        assert call(head, 0.07, outs, B, PK, P2, K2, D) == PH_EINVAL, (B, PK, P2, K2, D)
