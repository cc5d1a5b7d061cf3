"""ph_crd_kmeans_centers (csrc/crd_kmeans.hip) through the C ABI, against tests/kmeans_emulation.py.

  exact class   integer banks in [-4, 4] with duplicate rows and equal distances, iters = 1, k in {2, 3, 8}; one call holds classes
                of k, k + 1, 255, 256, 257, 513 rows, one of identical rows (empty clusters), one smaller than k, an empty one and
                one of offset rows: labels (and through them the picks of the initialisation), counts and centres bit for bit,
                centres = float32(float64 sum / count).
  real class    the seeded cases of tests/test_kmeans_emulation_cpu.py (257 / 513 / 1030 rows, k in {2, 3, 7}, iters in
                {1, 5, 16}): labels and counts equal to the float64 reference, centres bitwise equal to the float32 restatement
                and within 4 x the restatement's own error of the float64 reference (no transcendental: no device floor).
  fixed point   a converged case gives identical bits at iters 8 and 16, and two calls give identical bits.
  arguments     every PH_EINVAL with every output still holding its fill.

Outputs sit between sentinel guard bands, NaN-filled (centre rows) or -7-filled (labels, counts); the workspace is sized exactly by
ph_crd_kmeans_centers_workspace_bytes and guarded; the n_data bank rows are bitwise untouched."""
import numpy as np
import pytest
import torch

from tests import kmeans_emulation as E
from tests.gpu_util import Guarded

pytestmark = pytest.mark.gpu

D, UNWRITTEN = E.D, -7
_REF = {}


def _api():
    from multimodal_learning_amd._lib import lib, ptr, stream
    return lib(), ptr, stream()


def _reference(kind, k, T):
    """The float64 reference and the float32 restatement of a case, computed once."""
    key = (kind, k, T)
    if key not in _REF:
        case = {"exact": E.exact_inputs, "real": E.real_inputs}[kind](k) if kind != "fixed" else E.fixed_point_inputs()
        _REF[key] = (case, E.kmeans_pair(case, T, False), E.kmeans_pair(case, T, True))
    return _REF[key]


def _call(case, T, k=None, labels=True, counts=True, feat_dim=D, null=(), num_classes=None, expect=0):
    """One call on guarded buffers -> (return code, dict of numpy outputs, list of complaints)."""
    L, ptr, st = _api()
    k = case["k"] if k is None else k
    kk = min(max(k, 1), E.KMAX)                     # the buffers of an argument-error call are sized for a legal k
    n, C, total = case["n_data"], len(case["offsets"]) - 1, int(case["offsets"][-1])
    banks = []
    for b in ("bank1", "bank2"):
        M = Guarded((n + C * kk, D), torch.float32)
        M.t[:n].copy_(torch.from_numpy(case[b]).cuda())
        banks.append(M)
    lab = Guarded((2, total), torch.int32, fill=UNWRITTEN)
    cnt = Guarded((2, C, kk), torch.int32, fill=UNWRITTEN)
    nbytes = L.ph_crd_kmeans_centers_workspace_bytes(C, case["max_rows"], kk)
    assert nbytes > 0 and nbytes % 4 == 0
    W = Guarded((nbytes // 4,), torch.float32)
    members, offsets = torch.from_numpy(case["members"]).cuda(), torch.from_numpy(case["offsets"]).cuda()
    args = dict(mem1=ptr(banks[0].t), mem2=ptr(banks[1].t), members=ptr(members), offsets=ptr(offsets), workspace=ptr(W.t))
    for name in null:
        args[name] = None
    rc = L.ph_crd_kmeans_centers(args["mem1"], args["mem2"], args["members"], args["offsets"], C if num_classes is None else num_classes,
                                 case["max_rows"], n, feat_dim, k, T, ptr(lab.t) if labels else None, ptr(cnt.t) if counts else None,
                                 args["workspace"], st)
    torch.cuda.synchronize()
    bad = []
    for what, G in (("bank 1", banks[0]), ("bank 2", banks[1]), ("labels", lab), ("counts", cnt), ("workspace", W)):
        if not G.guards_intact():
            bad.append(f"{what}: guard band overwritten")
    out = dict(ext=np.stack([M.t.cpu().numpy() for M in banks]), labels=lab.t.cpu().numpy(), counts=cnt.t.cpu().numpy(),
               workspace=W.t.cpu().numpy())
    for b in range(2):
        if not np.array_equal(out["ext"][b, :n].view(np.int32), case["bank%d" % (b + 1)].view(np.int32)):
            bad.append(f"bank {b + 1}: the n_data bank rows changed")
    out["centres"] = out["ext"][:, n:].reshape(2, C, kk, D)
    assert rc == expect, (rc, expect)
    return rc, out, bad


def _bits(what, got, exp, bad):
    got, exp = np.ascontiguousarray(got), np.ascontiguousarray(exp)
    assert got.shape == exp.shape and got.dtype == exp.dtype, (what, got.shape, exp.shape, got.dtype, exp.dtype)
    same = got.view(np.int32) == exp.view(np.int32)
    if not same.all():
        i = tuple(int(v[0]) for v in np.nonzero(~same))
        bad.append(f"{what}: {int((~same).sum())} of {same.size} elements differ, first at {i}: got {got[i]!r} expected {exp[i]!r}")


def _written(out, bad):
    if np.isnan(out["centres"]).any():
        bad.append(f"centres: {int(np.isnan(out['centres']).sum())} elements never written (or NaN)")
    for key in ("labels", "counts"):
        if (out[key] == UNWRITTEN).any():
            bad.append(f"{key}: {int((out[key] == UNWRITTEN).sum())} elements never written")


@pytest.mark.parametrize("k", E.EXACT_K)
def test_exact_class(k):
    case, ref, rest = _reference("exact", k, 1)
    _, out, bad = _call(case, 1)
    _written(out, bad)
    _bits("labels", out["labels"], ref["labels"], bad)
    _bits("counts", out["counts"], ref["counts"], bad)
    _bits("centres", out["centres"], ref["centres"].astype(np.float32), bad)
    assert np.array_equal(rest["centres"], ref["centres"].astype(np.float32))
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("T", E.REAL_ITERS)
@pytest.mark.parametrize("k", E.REAL_K)
def test_real_class(k, T):
    case, ref, rest = _reference("real", k, T)
    _, out, bad = _call(case, T)
    _written(out, bad)
    _bits("labels", out["labels"], ref["labels"], bad)
    _bits("counts", out["counts"], ref["counts"], bad)
    _bits("centres against the float32 restatement", out["centres"], rest["centres"], bad)
    e_rest = float(np.abs(rest["centres"] - ref["centres"]).max())
    e_dev = float(np.abs(out["centres"] - ref["centres"]).max())
    print(f"k={k} T={T}: max |centre - float64 reference|: device {e_dev:.3e}, restatement {e_rest:.3e}")
    if e_dev > 4 * e_rest:
        bad.append(f"centres: error {e_dev:.3e} above 4 x the restatement's {e_rest:.3e}")
    assert not bad, "\n".join(bad)


def test_fixed_point_and_repeatability():
    case, ref, rest = _reference("fixed", 3, 8)
    assert all(E.stable_from(tr) is not None and E.stable_from(tr) <= 6 for b in range(2) for tr in ref["trace"][b])
    bad = []
    _, a, bad_a = _call(case, 8)
    _, b, bad_b = _call(case, 16)
    _, c, bad_c = _call(case, 16)
    for o in (a, b, c):
        _written(o, bad)
    for key in ("centres", "labels", "counts"):
        _bits(f"{key}: iters 8 against iters 16", a[key], b[key], bad)
        _bits(f"{key}: second call", c[key], b[key], bad)
    _bits("labels", a["labels"], ref["labels"], bad)
    _bits("centres against the float32 restatement", a["centres"], rest["centres"], bad)
    assert not (bad + bad_a + bad_b + bad_c), "\n".join(bad + bad_a + bad_b + bad_c)


def test_optional_outputs_may_be_null():
    case, ref, rest = _reference("fixed", 3, 8)
    _, out, bad = _call(case, 8, labels=False, counts=False)
    assert (out["labels"] == UNWRITTEN).all() and (out["counts"] == UNWRITTEN).all()
    _bits("centres", out["centres"], rest["centres"], bad)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("kw", [dict(feat_dim=64), dict(k=1), dict(k=9), dict(T=0), dict(num_classes=0), dict(null=("mem1",)),
                                dict(null=("mem2",)), dict(null=("members",)), dict(null=("offsets",)), dict(null=("workspace",))],
                         ids=lambda kw: "-".join(f"{a}={b}" for a, b in kw.items()))
def test_argument_errors_launch_nothing(kw):
    case = _reference("fixed", 3, 8)[0]
    kw = dict(kw)
    T = kw.pop("T", 4)
    _, out, bad = _call(case, T, expect=-22, **kw)
    assert np.isnan(out["centres"]).all() and np.isnan(out["workspace"]).all()
    assert (out["labels"] == UNWRITTEN).all() and (out["counts"] == UNWRITTEN).all()
    assert not bad, "\n".join(bad)
