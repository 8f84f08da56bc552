"""HIP-graph replay of an inference forward with fixed shapes.

The reference runs its small configurations (Cora: one 2708-node graph; PROTEINS: batch_size = 1, finetune-rag.py:27) as
a dozen eager launches per forward, and so does this package's eager path: at that size the forward is bound by the
host's launch rate (~0.14 ms of Python + HIP launches for ~0.07 ms of GPU work on c3), not by any kernel.  Every entry of
the C ABI allocates nothing, never synchronises and reads nothing back (the bf16-filtered retrieval repairs overflowed
rows on the device), so the whole forward can be captured ONCE into a HIP graph and replayed:

    fwd = CapturedForward(lambda x: model(x, adj), features)      # capture (model.eval(), fixed shapes, bank built)
    out = fwd(new_features)                                       # copy into the static input + one graph launch

The result tensor is the graph's static output buffer (clone it to keep it across calls).  Anything the forward reads
besides the captured inputs -- a closed-over CSRGraph, the bank, the weights -- is read from the same device addresses at
every replay: update those tensors in place, and re-capture after a bank grows (add_resources reallocates).

The adjacency may be a captured input too, in the reference's DENSE form:

    fwd = CapturedForward(lambda x, a: model(x, a), features, dense_adj)   # dense_adj fp32 [n, n], n <= K.ROW_BLOCK
    out = fwd(new_features, new_dense_adj)                                 # same padded size, any pattern

Every replay then converts the adjacency on the device (ragraph_dense_to_csr_f32: count, scan, fill -- no read-back) into
col / val buffers of n * n slots behind true row pointers (CSRGraph.padded), which the inference kernels walk by the row
pointers alone.  Graphs of different sizes share one capture when they are padded with zero rows and columns to one n: a
padded node has no edges, and its output rows are the caller's to ignore.  The conversion costs a few launches per replay
(profiles/dense_to_csr.txt): a caller whose adjacency never changes still does better closing over a CSRGraph.
"""
from __future__ import annotations

import torch


class CapturedForward:
    def __init__(self, fn, *example_inputs: torch.Tensor, warmup: int = 2):
        if not example_inputs or not all(isinstance(t, torch.Tensor) and t.is_cuda for t in example_inputs):
            raise ValueError("CapturedForward: the example inputs must be ROCm device tensors")
        self._fn = fn
        self.static_inputs = [t.clone() for t in example_inputs]
        cur = torch.cuda.current_stream()
        side = torch.cuda.Stream()
        side.wait_stream(cur)
        with torch.no_grad():
            with torch.cuda.stream(side):
                for _ in range(max(warmup, 1)):   # workspaces, LDS attributes, caches: everything lazy happens here
                    fn(*self.static_inputs)
            cur.wait_stream(side)
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph):
                self.static_output = fn(*self.static_inputs)

    def __call__(self, *inputs: torch.Tensor):
        if len(inputs) != len(self.static_inputs):
            raise ValueError(f"CapturedForward: expected {len(self.static_inputs)} inputs, got {len(inputs)}")
        for dst, src in zip(self.static_inputs, inputs):
            if src.shape != dst.shape or src.dtype != dst.dtype:
                raise ValueError(f"CapturedForward: input of shape {tuple(src.shape)} / {src.dtype}, captured with "
                                 f"{tuple(dst.shape)} / {dst.dtype} (re-capture for a new shape)")
            if src.data_ptr() != dst.data_ptr():
                dst.copy_(src, non_blocking=True)
        self.graph.replay()
        return self.static_output


class CapturedTrainStep:
    """A whole fine-tuning step -- forward, loss, backward, optimizer.step() -- captured ONCE into a HIP graph:

        def step(x, y):
            return torch.nn.functional.cross_entropy(model(x, adj), y)
        opt = torch.optim.Adam(model.parameters(), lr=1e-3, capturable=True)
        train = CapturedTrainStep(step, opt, features, labels)
        for x, y in batches:                      # fixed shapes
            loss = train(x, y)                    # copies into the static inputs + one graph launch, no sync

    `step_fn(*inputs)` returns the scalar loss.  Every parameter group must be `capturable=True` (torch's Adam / AdamW:
    their step counter lives on the device).  Warm-up runs eagerly on a side stream (workspaces, transposed graphs,
    normalised adjacencies: everything lazy happens there); afterwards every parameter, gradient and optimizer state is
    put back, so the first call is step 1 of the run an eager loop would make from the same state.  A step that
    synchronises (a read-back, a host-made tensor) fails the capture: RagraphNativeError with the cause, model and
    optimizer as they were.  The graph reads the parameters, the optimizer state and the retrieval banks at their capture
    addresses: after a bank grows or a parameter / state tensor is replaced the next call raises (re-capture)."""

    def __init__(self, step_fn, optimizer, *example_inputs: torch.Tensor, warmup: int = 3):
        from ._native import RagraphNativeError
        from .ragraph_utils.ToyGraphBase import _Bank

        if not example_inputs or not all(isinstance(t, torch.Tensor) and t.is_cuda for t in example_inputs):
            raise ValueError("CapturedTrainStep: the example inputs must be ROCm device tensors")
        for gi, group in enumerate(optimizer.param_groups):
            if not group.get("capturable", False):
                raise ValueError(f"CapturedTrainStep: parameter group {gi} of {type(optimizer).__name__} is not "
                                 "capturable=True (its step counter would be read on the host)")
        params = [p for group in optimizer.param_groups for p in group["params"]]
        fresh = [p for p in params if not optimizer.state.get(p)]
        if fresh and not isinstance(optimizer, (torch.optim.Adam, torch.optim.AdamW)):
            raise ValueError("CapturedTrainStep: the state of a fresh optimizer is restored as zeros after warm-up, which "
                             "is Adam's / AdamW's initial state only: take one of those, or run one eager step first")
        self._fn, self._opt, self._params = step_fn, optimizer, params
        self.static_inputs = [t.clone() for t in example_inputs]
        # what the warm-up changes, to be put back: parameters, gradients, optimizer state, the device RNG
        saved_p = [p.detach().clone() for p in params]
        saved_g = [None if p.grad is None else p.grad.detach().clone() for p in params]
        saved_s = {p: {k: (v.detach().clone() if isinstance(v, torch.Tensor) else v) for k, v in optimizer.state[p].items()}
                   for p in params if optimizer.state.get(p)}
        rng, rng_host = torch.cuda.get_rng_state(), torch.random.get_rng_state()

        def restore(final: bool):
            """final=False: the state to capture from -- a state the warm-up created for a fresh optimizer stays (the
            graph needs its tensors) and is zeroed, Adam's / AdamW's state before a first step.  final=True (giving
            up): exactly as before the constructor -- created states dropped, gradients put back."""
            with torch.no_grad():
                for p, s in zip(params, saved_p):
                    p.copy_(s)
                for p in params:
                    st = optimizer.state.get(p)
                    if not st:
                        continue
                    old = saved_s.get(p)
                    if old is None and final:
                        optimizer.state.pop(p)
                        continue
                    for k, v in st.items():
                        if isinstance(v, torch.Tensor):
                            if old is None:
                                v.zero_()
                            else:
                                v.copy_(old[k])
                        elif old is not None and k in old:
                            st[k] = old[k]
                if final:
                    for p, g in zip(params, saved_g):
                        p.grad = None if g is None else g.clone()
            torch.cuda.set_rng_state(rng)
            torch.random.set_rng_state(rng_host)

        cur = torch.cuda.current_stream()
        side = torch.cuda.Stream()
        side.wait_stream(cur)
        _Bank.reads = {}
        try:
            with torch.cuda.stream(side):
                for _ in range(max(warmup, 1)):
                    optimizer.zero_grad(set_to_none=True)
                    step_fn(*self.static_inputs).backward()
                    optimizer.step()
            cur.wait_stream(side)
            banks = list(_Bank.reads.values())
        except BaseException:
            cur.wait_stream(side)
            restore(final=True)
            raise
        finally:
            _Bank.reads = None
        from .layers.gcn import sparse_features
        for i, t in enumerate(self.static_inputs):
            if sparse_features(t, probe=False) is not None:
                restore(final=True)
                raise ValueError(f"CapturedTrainStep: input {i} is a bag-of-words feature matrix multiplied through its "
                                 "CSR form, which is made once per tensor on the host side: a replay would keep the "
                                 "capture-time CSR.  Close over fixed features in step_fn instead of passing them")
        restore(final=False)
        self._banks = [(b, b.buf.data_ptr(), b.n) for b in banks]
        self.graph = torch.cuda.CUDAGraph()
        try:
            with torch.cuda.graph(self.graph):
                # a synchronising call must fail HERE, on the host, before the runtime sees it inside the capture
                mode = torch.cuda.get_sync_debug_mode()
                torch.cuda.set_sync_debug_mode("error")
                try:
                    optimizer.zero_grad(set_to_none=True)
                    self.static_loss = step_fn(*self.static_inputs)
                    self.static_loss.backward()
                    optimizer.step()
                finally:
                    torch.cuda.set_sync_debug_mode(mode)
        except Exception as e:
            self.graph = None
            restore(final=True)
            raise RagraphNativeError(f"CapturedTrainStep: the step could not be captured ({type(e).__name__}: {e})") from e
        self._addrs = self._addresses()

    def _addresses(self):
        out = [p.data_ptr() for p in self._params]
        for p in self._params:
            out += [v.data_ptr() for v in self._opt.state.get(p, {}).values() if isinstance(v, torch.Tensor)]
        return out

    def __call__(self, *inputs: torch.Tensor):
        from ._native import RagraphNativeError

        if len(inputs) != len(self.static_inputs):
            raise ValueError(f"CapturedTrainStep: expected {len(self.static_inputs)} inputs, got {len(inputs)}")
        for b, ptr, n in self._banks:
            if b.buf.data_ptr() != ptr or b.n != n:
                raise RagraphNativeError("CapturedTrainStep: a retrieval bank the step reads has grown since the capture "
                                         f"({n} -> {b.n} rows): re-capture")
        if self._addresses() != self._addrs:
            raise RagraphNativeError("CapturedTrainStep: a parameter or optimizer state tensor was replaced since the "
                                     "capture (the graph holds the old addresses): re-capture")
        for dst, src in zip(self.static_inputs, inputs):
            if src.shape != dst.shape or src.dtype != dst.dtype:
                raise ValueError(f"CapturedTrainStep: input of shape {tuple(src.shape)} / {src.dtype}, captured with "
                                 f"{tuple(dst.shape)} / {dst.dtype} (re-capture for a new shape)")
            if src.data_ptr() != dst.data_ptr():
                dst.copy_(src, non_blocking=True)
        self.graph.replay()
        return self.static_loss
