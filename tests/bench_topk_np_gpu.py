"""Timing of ph_crd_bank_topk (the MIA-2023 KNN) over the number of neighbours (not a pytest file):

    python tests/bench_topk_np_gpu.py [--parent PATH --parent PATH] [--widths 64 128 256] [--num-pos 6 8 ...] [--rounds N] [--seconds S]

65 536 rows x 64 queries, num_pos in {6, 8, 9, 16, 32, 64}, at each width.  Device events around back-to-back calls, warmed
up, the repeat count chosen so that a figure is at least --seconds of device work.

--parent names builds of libpathomic_hip.so from the parent commit (two copies of one build under different file names, so that
the loader keeps them apart).  At num_pos 6 and 8 they are timed alternately with this build, round by round, in one process on one
device, and the outputs are compared bit for bit.  Two statements are checked and reported:

  num_pos <= 8   this build lies inside the spread of the parent against itself (min .. max over both copies and all rounds,
                 widened by nothing);
  num_pos > 8    the call costs no more than ceil(num_pos / 8) times the parent's num_pos = 8 call (its mean) - sample pass and
                 thresholds run once, so it should cost less."""
import argparse
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch            # noqa: E402

from multimodal_learning_amd import _lib      # noqa: E402

N, B = 65536, 64
NUM_POS = (6, 8, 9, 16, 32, 64)


def load(path, np_size):
    l = C.CDLL(path)
    for name in ("ph_crd_bank_topk", "ph_crd_bank_topk_workspace_bytes") + (("ph_crd_bank_topk_workspace_bytes_np",) if np_size else ()):
        fn = getattr(l, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    return l


def timed(call, min_seconds):
    for _ in range(20):
        call()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(50):
        call()
    e1.record(); torch.cuda.synchronize()
    reps = max(50, int(min_seconds * 1e3 / (e0.elapsed_time(e1) / 50)) + 1)
    e0.record()
    for _ in range(reps):
        call()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


class Scan:
    def __init__(self, D, NP, ws_bytes):
        g = torch.Generator().manual_seed(2)
        self.D, self.NP = D, NP
        self.mem = [(torch.rand(N, D, generator=g) - 0.5).cuda() for _ in range(2)]
        self.labels = torch.randint(0, 3, (N,), generator=g).int().cuda()
        self.idx = torch.randint(0, N, (B, 5), generator=g).cuda()
        self.bl = self.labels[self.idx[:, 0]].long()
        self.nb = [torch.empty(B, NP, dtype=torch.int64, device="cuda") for _ in range(2)]
        self.sim = [torch.empty(B, NP, device="cuda") for _ in range(2)]
        self.ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")

    def call(self, L):
        p = _lib.ptr
        return L.ph_crd_bank_topk(p(self.mem[0]), p(self.mem[1]), p(self.labels), p(self.idx), 5, p(self.bl), B, N, self.NP, self.D,
                                  p(self.nb[0]), p(self.nb[1]), p(self.sim[0]), p(self.sim[1]), p(self.ws), _lib.stream())

    def outputs(self, L):
        for t in self.nb + self.sim:
            t.zero_()
        assert self.call(L) == 0
        torch.cuda.synchronize()
        return b"".join(t.cpu().numpy().tobytes() for t in self.nb + self.sim)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", action="append", default=[])
    ap.add_argument("--widths", type=int, nargs="+", default=[64, 128, 256])
    ap.add_argument("--num-pos", type=int, nargs="+", default=list(NUM_POS))
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seconds", type=float, default=0.5)
    a = ap.parse_args()
    this = load(_lib.LIB_PATH, True)
    parents = [load(p, False) for p in a.parent]
    print("this build = %s" % _lib.LIB_PATH)
    for k, p in enumerate(a.parent):
        print("parent %d = %s" % (k, p))
    findings = []
    for D in a.widths:
        parent8 = None
        for NP in a.num_pos:
            w = Scan(D, NP, this.ph_crd_bank_topk_workspace_bytes_np(B, N, NP))
            assert w.call(this) == 0
            torch.cuda.synchronize()
            if NP <= 8 and parents:
                assert this.ph_crd_bank_topk_workspace_bytes_np(B, N, NP) == parents[0].ph_crd_bank_topk_workspace_bytes(B, N)
                same = all(w.outputs(P) == w.outputs(this) for P in parents)
                tp, tt = [], []
                for r in range(a.rounds):
                    for P in parents:
                        tp.append(timed(lambda: w.call(P), a.seconds))
                    tt.append(timed(lambda: w.call(this), a.seconds))
                inside = min(tp) <= sum(tt) / len(tt) <= max(tp)
                print("D %3d num_pos %2d: parent %s us | this build %s us | outputs %s | mean of this build %s the parent's spread"
                      % (D, NP, " ".join("%.2f" % t for t in tp), " ".join("%.2f" % t for t in tt),
                         "bit for bit the parent's" if same else "DIFFERENT", "inside" if inside else "OUTSIDE"), flush=True)
                if not same:
                    findings.append("D %d num_pos %d: outputs differ from the parent build's" % (D, NP))
                if not inside:
                    findings.append("D %d num_pos %d: %.2f us outside the parent's %.2f .. %.2f us" % (D, NP, sum(tt) / len(tt), min(tp), max(tp)))
                if NP == 8:
                    parent8 = sum(tp) / len(tp)
            else:
                tt = [timed(lambda: w.call(this), a.seconds) for r in range(a.rounds)]
                us = sum(tt) / len(tt)
                if NP == 8:
                    parent8 = us      # (no parent build given: this build's own num_pos = 8 call)
                line = "D %3d num_pos %2d: this build %s us" % (D, NP, " ".join("%.2f" % t for t in tt))
                if NP > 8 and parent8:
                    npass = (NP + 7) // 8
                    line += " | %.2f x the num_pos = 8 call (%.2f us), bound %d" % (us / parent8, parent8, npass)
                    if us > npass * parent8:
                        findings.append("D %d num_pos %d: %.2f us > %d x %.2f us" % (D, NP, us, npass, parent8))
                print(line, flush=True)
    print("findings: %s" % ("none" if not findings else ""))
    for f in findings:
        print("  " + f)


if __name__ == "__main__":
    main()
