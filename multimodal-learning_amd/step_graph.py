"""HIP-graph replay of a training step, shared by DistillStep and TeacherStage1Step (train_step.py): which input set serves a
batch (`select_set`, plain values, no GPU needed) and the capture of one graph per input set and kind of step (`StepGraphs`).

A captured graph reads its inputs from the addresses it was captured with.  Device-resident, contiguous inputs (a loader's ring
of batch buffers) are ADOPTED as they are, up to two sets, and replayed without a copy; host tensors or further resident sets
are copied into ONE private set of buffers - never into an adopted set, whose tensors belong to the caller."""
import warnings

import torch

from ._lib import lib

MAX_ADOPTED = 2


def select_set(sets, resident, ptrs, shapes, stage=True):
    """The input set that serves a batch: -> (record, new, copy).  `sets`: the list of records so far, edited in place (emptied
    when `shapes` differs from the first record's; a new record is appended); `resident`: every input is a contiguous device
    tensor; `ptrs` / `shapes`: their data pointers / shapes in input order.  A record is a dict with `shapes`, `ptrs`,
    `adopted`, `graphs` and `graph` (the graph captured last, None before the first); `new` asks the caller to attach the buffers (the given tensors if adopted, fresh ones and their
    `ptrs` otherwise) and `copy` to copy the inputs in.  A resident tuple is served by the set with its pointers (an adopted
    set, or the private one handed its own buffers back) or adopted while fewer than MAX_ADOPTED sets are; everything else goes
    to the private set - with `stage` False to no set at all (None, False, False)."""
    if sets and sets[0]["shapes"] != shapes:
        del sets[:]
    if resident:
        st = next((q for q in sets if q["ptrs"] == ptrs), None)
        if st is not None:
            return st, False, False
        if sum(q["adopted"] for q in sets) < MAX_ADOPTED:
            sets.append(dict(shapes=shapes, ptrs=ptrs, adopted=True, graphs={}, graph=None))
            return sets[-1], True, False
    if not stage:
        return None, False, False
    st = next((q for q in sets if not q["adopted"]), None)
    if st is not None:
        return st, False, True
    sets.append(dict(shapes=shapes, ptrs=None, adopted=False, graphs={}, graph=None))
    return sets[-1], True, True


def capture_mode(sync):
    """Stream-capture error mode of the step graphs.  Under data parallelism the process group's watchdog thread keeps polling
    the completion events of earlier collectives (hipEventQuery); in the default "global" mode that call from ANOTHER thread is
    illegal while a capture runs and takes the process down (seen intermittently with `bench.py --force-dist`): "thread_local"
    restricts the check to the capturing thread.  Kernels enqueued on the capturing stream by other threads (autograd's
    backward worker) are captured either way."""
    return "thread_local" if sync is not None else "global"


class StepGraphs:
    """The input sets of one step object and their captured graphs.  A set is the record of `select_set` plus its input
    tensors under their names (`names`; the same dict as `bufs`) and whatever the step keeps with it; `graphs` maps the kind
    of step to (graph, outputs, workspace references).  `nets`: the networks whose trunk workspaces the graphs point into.
    Behaves as the list of its sets.  It holds no reference to the step: the step owns it, and a cycle between the two would
    leave the graphs to the garbage collector, which may then destroy them in the middle of a later capture."""

    def __init__(self, device, what, names, nets):
        self.device, self.what, self.names, self.nets = device, what, names, nets
        self.sets = []

    def __len__(self):
        return len(self.sets)

    def __getitem__(self, i):
        return self.sets[i]

    def input_set(self, given, stage=True):
        """The set that serves the tensors `given` (by name), filled with them; None if `stage` is False and they would have
        to be copied."""
        vals = [given[k] for k in self.names]
        resident = all(t.is_cuda and t.is_contiguous() for t in vals)
        ptrs = tuple(t.data_ptr() for t in vals) if resident else None
        st, new, copy = select_set(self.sets, resident, ptrs, tuple(tuple(t.shape) for t in vals), stage)
        if new:      # adopted: the caller refills these tensors in place
            bufs = {k: t if st["adopted"] else torch.empty(t.shape, device=self.device, dtype=t.dtype) for k, t in zip(self.names, vals)}
            st.update(bufs, bufs=bufs, ptrs=tuple(t.data_ptr() for t in bufs.values()))
        if copy:
            for k, t in zip(self.names, vals):
                st[k].copy_(t, non_blocking=True)
        return st

    def graph(self, owner, st, kind, body, first=None, before=None):
        """(graph, outputs) of the step `kind` of `owner` (sync, optimizer, _want_graph) on the set `st`, captured from `body()`
        on first need - after `before()`, which allocates what must not be allocated under capture, and with `first()`
        captured in front.  None if the capture failed: every set is dropped and the owner launches eagerly from now on."""
        if kind not in st["graphs"]:
            optimizer = owner.optimizer
            lib().ph_prof_enable(0)          # event timing is an eager-mode facility
            g = torch.cuda.CUDAGraph()
            torch.cuda.synchronize()
            pool = next((gr.pool() for q in self.sets for gr, _, _ in q["graphs"].values()), None)
            was_prepared = optimizer._prepared
            try:
                if before is not None:
                    before()
                with torch.cuda.graph(g, pool=pool, capture_error_mode=capture_mode(owner.sync)):
                    optimizer._prepared = True            # the step scalars are read from device memory at replay
                    if first is not None:
                        first()
                    out = body()
                # the graph holds raw pointers into the trunk workspaces it was captured with: keep them alive with it
                refs = [ws for net in self.nets for mod in net.modules() if hasattr(mod, "pinned_workspaces")
                        for ws in mod.pinned_workspaces()]
                st["graphs"][kind] = (g, out, refs)
                st["graph"] = g
                optimizer._prepared = was_prepared        # capture does not execute anything
            except Exception as exc:     # e.g. a collective that cannot be captured on this stack: stay eager
                warnings.warn("HIP graph capture of the %s step failed (%r); continuing with eager launches" % (self.what, exc))
                torch.cuda.synchronize()
                try:      # on this HIP runtime a failed capture can leave its streams in capture state for good
                    torch.ones(1).to(self.device)
                except Exception as exc2:
                    raise RuntimeError("HIP graph capture of the %s step failed (%r) and the runtime did not leave capture "
                                       "mode (%r): restart the process without enable_graph()" % (self.what, exc, exc2)) from exc
                owner._want_graph = False
                del self.sets[:]
                optimizer._prepared = was_prepared
                return None
        return st["graphs"][kind][:2]
