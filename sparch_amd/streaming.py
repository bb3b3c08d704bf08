"""
Streaming inference: a trained spiking network classifies a stream chunk by chunk, carrying every neuron's state
from one chunk to the next.

    st = StreamingSNN(net, batch_size)          # net.eval(), unidirectional
    st.reset()                                  # the draws one SNN.forward would make, same generator, same order
    out = st.step(x_chunk)                      # (B,Tc,C), any Tc >= 1 -> running softmax-sum (B,classes)

What is carried per hidden layer is (u, [w,] s) after the chunk's last step, per readout (u, out): a step of the cell
recurrences needs nothing else, and the arithmetic of a step does not know where a chunk ends — so the spikes of a
chunked stream are those of one forward over the whole sequence, bit for bit wherever the matrix products are exact
(dyadic weights), and the readout's running sum continues ONE sequential sum over t (the accumulator goes into the
kernel; adding per-chunk sums would round differently).  The kernels are the `*_stream_fwd` entry points of the
library: state in, state out, in place, no (B,T,H) save tensors.

Everything a forward call derives from the parameters alone — the split planes of W, the packed and masked V, the
eval-mode BatchNorm fold — is made once (`refresh()` after the parameters change); a chunk step launches the
projection, the boundary product s @ V of a recurrent layer and the cell, nothing else.

    st = StreamingSNN(net, batch_size, fused=True)

serves the chunk of ONE time step (a live stream) with one launch per layer: `sparch_stream_step_fwd` does the
projection, the BatchNorm affine, s @ V and the cell for a hidden layer, `sparch_stream_step_readout` the readout
(csrc/streamstep.hip).  Every workgroup of a recurrent layer reads all of the previous spikes, so those layers keep
their spike state twice and the host swaps which copy is current after each fused step.  Longer chunks take the
path above on the same state.

    st = StreamingSNN(net, batch_size, fused=True, sparse=True)

makes the fused step event-driven: `sparch_stream_step_sparse_fwd` / `sparch_stream_step_sparse_readout`
(csrc/streamsparse.hip) list the non-zero inputs of every row and read only their rows of the transposed weights
(`W.t()` and the un-transposed masked V, cached by `refresh()`), about nnz * H * 4 bytes per operand instead of all of
W and V.  Same state, same buffer swap, same launches per step; leaving out zero inputs changes no sum, only the order
of the non-zero terms differs from the dense fused step.
"""
import numpy as np
import torch

from . import functional as Fn
from ._capi import KIND, check, lib, ptr


def _transposed(W):
    """W (H,K) -> W^T (K, ldw) fp32, ldw = H rounded up to a multiple of 4 (zero-padded): one contiguous row per input."""
    H = W.shape[0]
    return _pad_cols(W.t(), (H + 3) // 4 * 4).contiguous()


def _pad_cols(t, H4):
    return None if t is None else torch.nn.functional.pad(t, (0, H4 - t.shape[-1]))


class _Layer:
    """One layer's cached operands and its state buffers (plain attribute bag)."""


class _ParityGraphs(dict):
    """graph=True, steps of one time step: {what identifies the current copy of the state: dict(graph, replays)}, one
    captured chain of launches per parity, with the static input and output they share."""

    def __init__(self):
        super().__init__()
        self.x = self.out = self.dtype = None
        self.warm = 0


class _Stream:
    """What StreamingSNN and StreamingANN share: the refusals, the step counts, the chunk check, the checked load of a
    state tensor, the BatchNorm fold and the replayed single step on two copies of the state.  A subclass refuses the
    wrong kind of network first, sets `_layers` and `_dev` in refresh(), and for graph=True provides `_state_key()` and
    `_static_step(x)`."""

    def __init__(self, net, batch_size, graph):
        name = type(self).__name__
        if net.bidirectional:
            raise ValueError(f"{name}: a bidirectional network is not causal — its backward direction needs "
                             "the end of the sequence before the first output")
        if net.training:
            raise ValueError(f"{name}: the network is in training mode — BatchNorm's batch statistics and "
                             "dropout have no streaming meaning; call net.eval() first")
        self.net = net
        self.batch_size = int(batch_size)
        self.graph = bool(graph)
        self.steps_seen = 0
        self.row_steps = np.zeros(self.batch_size, dtype=np.int64)
        self._layers = None

    def _restart(self, rows):
        if rows is None:
            self.steps_seen = 0
            self.row_steps[:] = 0
        else:
            self.row_steps[list(rows)] = 0

    def _chunk(self, x):
        """The checked chunk (B,Tc,K) on the device, a 4-D one flattened when net.reshape."""
        if self.net.reshape and x.ndim == 4:
            x = x.reshape(x.shape[0], x.shape[1], x.shape[2] * x.shape[3])
        Fn._require_device(x, "input")
        K = self._layers[0].K
        if x.ndim != 3 or x.shape[0] != self.batch_size or x.shape[1] < 1 or x.shape[2] != K:
            raise ValueError(f"{type(self).__name__}.step: a ({self.batch_size}, Tc >= 1, {K}) chunk, got "
                             f"{tuple(x.shape)}")
        return x

    def _rows(self, rows):
        return None if rows is None else torch.as_tensor(list(rows), dtype=torch.long, device=self._dev)

    def _entries(self, states):
        if len(states) != len(self._layers):
            raise ValueError(f"{type(self).__name__}: {len(self._layers)} layers, {len(states)} state entries")
        return zip(self._layers, states)

    def _put(self, dst, src, what, idx, H=None):
        """src (all rows, or the rows idx) -> the state tensor dst; H: the layer's own width where dst is padded."""
        name, H = type(self).__name__, dst.shape[1] if H is None else H
        n = self.batch_size if idx is None else len(idx)
        if src is None:
            raise ValueError(f"{name}: the state has no {what}")
        src = torch.as_tensor(src, dtype=torch.float32).to(self._dev)
        if src.ndim != 2 or src.shape[0] != n or src.shape[1] not in (H, dst.shape[1]):
            raise ValueError(f"{name}: {what} has shape {tuple(src.shape)}, expected ({n}, {H})")
        src = _pad_cols(src, dst.shape[1])
        if idx is None:
            dst.copy_(src)
        else:
            dst.index_copy_(0, idx, src)

    def set_state(self, states):
        """Load a state (the format of get_state(), or of reset(states=...)) without touching the counters."""
        self._ensure()
        self._load(states, None)

    def _bn_fold(self, H, norm):
        """Eval BatchNorm: the running statistics folded into one affine map (scale, shift) per column."""
        _, scale, shift, _ = Fn._Norm.forward(
            "batchnorm", torch.empty(1, H, dtype=torch.float32, device=self._dev), None, norm.weight, norm.bias,
            norm.running_mean, norm.running_var, False, 1)
        return scale, shift

    def _replayed_step(self, graphs, x):
        """Replay the captured chain of launches for the current copy of the state (captured on first need, after one
        eager step, for the first input dtype seen) on x -> the static output; None = launch eagerly.  The caller
        swaps the copies behind it."""
        if graphs.dtype is None:
            graphs.dtype = x.dtype
        if x.dtype != graphs.dtype:
            return None
        if graphs.warm < 1:
            graphs.warm += 1
            return None
        key = self._state_key()
        g = graphs.get(key)
        if g is None:
            if graphs.x is None:
                last = self._layers[-1]
                graphs.x = torch.empty(x.shape, dtype=x.dtype, device=self._dev)
                graphs.out = torch.empty((self.batch_size, last.H) if last.readout else (self.batch_size, 1, last.H),
                                         dtype=torch.float32, device=self._dev)
            g = {"graph": torch.cuda.CUDAGraph(), "replays": 0}
            torch.cuda.synchronize()
            with torch.cuda.graph(g["graph"]):
                graphs.out.copy_(self._static_step(graphs.x))
            graphs[key] = g
        graphs.x.copy_(x, non_blocking=True)
        g["graph"].replay()
        g["replays"] += 1
        return graphs.out


class StreamingSNN(_Stream):
    """Chunked forward of a `sparch_amd.SNN` in eval mode with carried state.

    step(x_chunk) returns, with a readout layer, the running softmax-sum (B,classes) after all steps seen so far — or,
    on the chunk path, the network's own readout (SNN(readout=...)) of the steps seen so far: the mean over them, the
    running maximum, the last membrane; fused=True takes the default readout only —
    (with graph=True a static tensor that the next step overwrites), without one the chunk's spikes (B,Tc,H).
    firing_rates() is spike count / (B * steps_seen) per hidden unit, concatenated over the layers as SNN.forward
    does; the integer counts add exactly across chunks.  The spike counters are per layer, NOT per row:
    reset(rows=...) restarts the state, the running output and the step count of those rows and leaves the counters
    (and steps_seen) alone.  Nothing here synchronises with the device.

    A recurrent kernel whose in-kernel wait times out raises the status word (`functional.check_status`) as in the
    whole-sequence path; the stream kernels have by then written a half-advanced state over the carried one, so after
    such a report the stream can only be continued from a reset() (or a set_state() of a state saved earlier)."""

    def __init__(self, net, batch_size, graph=False, fused=False, sparse=False):
        if not getattr(net, "is_snn", False):
            raise ValueError("StreamingSNN: a sparch_amd.SNN (the non-spiking baselines do not stream)")
        super().__init__(net, batch_size, graph)
        if sparse and not fused:
            raise ValueError("StreamingSNN: sparse=True is a form of the fused one-step path — pass fused=True too")
        if fused and any(mod.normalize and mod.normalization == "layernorm" for mod in net.snn):
            raise ValueError("StreamingSNN: fused=True does not take LayerNorm layers (a row statistic across the "
                             "workgroups of a step); use fused=False")
        readout = self._readout_name(net)
        Fn.readout_mode(readout)
        if fused and readout != "softmax_sum":
            raise ValueError(f"StreamingSNN: fused=True does not take readout={readout!r} (the one-step readout kernels "
                             "are the softmax-sum's); use fused=False")
        # axonal delays (SNN(max_delay=...)): the chunk path carries one history of the last max_delay input steps per
        # delayed layer; the one-launch fused and event-driven steps and the captured chunk step do not
        self._has_delays = any(getattr(mod, "max_delay", 0) for mod in net.snn)
        if self._has_delays and (fused or sparse):
            raise ValueError("StreamingSNN: fused=True / sparse=True do not take a network with axonal delays (the "
                             "one-launch step has no delayed input); use fused=False")
        if self._has_delays and graph:
            raise ValueError("StreamingSNN: graph=True does not take a network with axonal delays (the captured chunk "
                             "step covers networks without them only); use graph=False")
        # synaptic currents (SNN(synapse=...)): the chunk path carries the current i (B,H) per layer; the same refusals
        self._has_synapse = any(getattr(mod, "synapse", None) is not None for mod in net.snn)
        if self._has_synapse and (fused or sparse):
            raise ValueError("StreamingSNN: fused=True / sparse=True do not take a network with synaptic currents (the "
                             "one-launch step has no filtered input); use fused=False")
        if self._has_synapse and graph:
            raise ValueError("StreamingSNN: graph=True does not take a network with synaptic currents (the captured chunk "
                             "step covers networks without them only); use graph=False")
        self.fused = bool(fused)
        self.sparse = bool(sparse)
        self._fused_active = self.fused and Fn._prec() == 0
        self._fg = _ParityGraphs()  # fused step, graph=True: keyed by the current spike buffers
        self._prec = None
        self._g = None            # dict(Tc, x, out, graph) once the step is captured
        self._g_Tc = None         # the chunk length the graph is (to be) captured for: the first one seen
        self._g_warm = 0
        self._g_replays = 0
        # inspection hook of the tests, not part of the interface: callable(layer_index, spikes (B,Tc,H)) called behind every chunk step for every hidden
        # layer with the chunk's spikes as they travel to the next layer (the bf16 0/1 plane); the tensor
        # is only valid during the call (graph=True: a static buffer the next replay overwrites)
        self._spike_tap = None

    @staticmethod
    def _readout_name(net):
        """The readout layer's reduction over time (snns.ReadoutLayer; a module from before the attribute: the default)."""
        return getattr(net.snn[-1], "readout", "softmax_sum") if net.use_readout_layer else "softmax_sum"

    # ------------------------------------------------------------------ caches
    def refresh(self):
        """(Re)build everything derived from the parameters and the running statistics: call after changing them.
        The state of the stream is kept."""
        net, B = self.net, self.batch_size
        dev = self._dev = next(net.parameters()).device
        Fn._require_device(next(net.parameters()), "the network")
        old = self._layers
        layers = []
        last = net.num_layers - 1
        with torch.no_grad():
            for i, mod in enumerate(net.snn):
                L = _Layer()
                L.readout = bool(net.use_readout_layer and i == last)
                L.kind = None if L.readout else mod.kind
                L.recurrent = L.kind in ("RLIF", "RadLIF")
                L.adaptive = L.kind in ("adLIF", "RadLIF")
                L.H, L.K = mod.hidden_size, mod.input_size
                L.W = Fn._f32c(mod.W.weight.detach())
                L.Wb = None if mod.W.bias is None else Fn._f32c(mod.W.bias.detach())
                L.w_planes = Fn.split_planes(L.W) if (L.K % 32 == 0 and L.H >= 128) else None
                L.Wt = _transposed(L.W) if self.sparse else None  # the event-driven step's operand: row k = input k
                L.norm = mod.normalization if mod.normalize else "none"
                L.scale = L.shift = L.nw = L.nb = None
                if L.norm == "batchnorm":
                    L.scale, L.shift = self._bn_fold(L.H, mod.norm)
                elif L.norm == "layernorm":
                    L.nw, L.nb = mod.norm.weight.detach(), mod.norm.bias.detach()
                L.theta = None if L.readout else float(mod.threshold)
                # axonal delays: the parameter, and (a state buffer, made at the first chunk in the dtype the layer's
                # input travels in) the last D input steps (B,D,K)
                L.D = int(getattr(mod, "max_delay", 0))
                L.delay = Fn._f32c(mod.delay.detach()) if L.D else None
                L.hist = None
                # synaptic currents: the limits, the parameter and the folded BatchNorm affine, which the filter applies
                # (the cell then reads the current with no scale and no shift); the carried current is L.i (B,H)
                L.syn = getattr(mod, "synapse", None)
                L.gamma = Fn._f32c(mod.gamma.detach()) if L.syn is not None else None
                L.syn_scale, L.syn_shift = (L.scale, L.shift) if L.syn is not None else (None, None)
                if L.syn is not None:
                    L.scale = L.shift = None
                L.i = None
                # readout: the reduction over time; the mean modes carry the un-normalised accumulator in `out` and the
                # rows' step counts in `steps`, u_max the running maximum (from -inf)
                L.red = Fn.readout_mode(self._readout_name(net)) if L.readout else 0
                L.red_mean = L.red in (Fn.READOUT_MODES["softmax_mean"], Fn.READOUT_MODES["u_mean"])
                L.out_init = float("-inf") if L.red == Fn.READOUT_MODES["u_max"] else 0.0
                # the recurrent kernels own 4 columns per thread: other widths run zero-padded (as cell_forward does),
                # and the padded state stays padded
                L.Hs = (L.H + 3) // 4 * 4 if L.recurrent else L.H
                pad = (lambda t: _pad_cols(t, L.Hs)) if L.Hs != L.H else (lambda t: t)
                L.p = {"alpha": pad(mod.alpha.detach())}
                if L.adaptive:
                    L.p.update(beta=pad(mod.beta.detach()), a=pad(mod.a.detach()), b=pad(mod.b.detach()))
                if L.Hs != L.H:
                    L.scale, L.shift = pad(L.scale), pad(L.shift)
                if L.recurrent:
                    V = Fn._f32c(mod.V.weight.detach())
                    if L.Hs != L.H:
                        V = torch.nn.functional.pad(V, (0, L.Hs - L.H, 0, L.Hs - L.H))
                    L.step_path = Fn.rec_step_path(L.Hs)
                    L.vmask = torch.empty(L.Hs, L.Hs, dtype=torch.float32, device=dev)
                    if L.step_path:
                        L.vpack = None
                        check(lib.sparch_vmask(L.Hs, ptr(V), ptr(L.vmask), Fn._stream()), "sparch_vmask")
                    else:
                        L.vpack = Fn._vpack(L.Hs, V, 0, vmask=L.vmask)
                    L.vmask_t = L.vmask.t().contiguous()  # (H_out, H_in): the NT operand of the exact spike product
                # state buffers: kept across refresh()
                if old is not None:
                    for k in ("u", "w", "s", "s16", "count", "out", "steps", "binary", "s_alt", "s16_alt", "s_first",
                              "hist", "i"):
                        setattr(L, k, getattr(old[i], k, None))
                    if L.syn is not None and L.i is None:
                        L.i = torch.zeros(B, L.H, dtype=torch.float32, device=dev)
                elif L.readout:
                    L.u = torch.zeros(B, L.H, dtype=torch.float32, device=dev)
                    L.out = torch.full((B, L.H), L.out_init, dtype=torch.float32, device=dev)
                    L.steps = torch.zeros(B, 1, dtype=torch.int32, device=dev) if L.red_mean else None
                else:
                    L.u = torch.zeros(B, L.Hs, dtype=torch.float32, device=dev)
                    L.w = torch.zeros(B, L.Hs, dtype=torch.float32, device=dev) if L.adaptive else None
                    L.s = torch.zeros(B, L.Hs, dtype=torch.float32, device=dev)
                    L.s16 = torch.zeros(B, L.Hs, dtype=torch.bfloat16, device=dev) if L.recurrent else None
                    L.count = torch.zeros(L.Hs, dtype=torch.int32, device=dev)
                    L.binary = False  # s holds 0/1 only AND s16 mirrors it (true behind every chunk step)
                    L.s_alt = L.s16_alt = L.s_first = None
                    if L.syn is not None:
                        L.i = torch.zeros(B, L.H, dtype=torch.float32, device=dev)
                if self.fused and L.recurrent and L.s_alt is None:
                    # the other copy of the spike state: a fused step reads s / writes s_alt, then the host swaps the
                    # names (its padded columns are never written: they stay zero like those of s)
                    L.s_alt, L.s16_alt, L.s_first = torch.zeros_like(L.s), torch.zeros_like(L.s16), L.s
                layers.append(L)
        self._layers, self._prec = layers, Fn._prec()
        self._g, self._g_warm = None, 0  # a captured step holds the old operands
        self._fg = _ParityGraphs()
        self._fused_active = self.fused and self._prec == 0  # (the bf16 operand mode takes the chunk path)

    @property
    def fused_active(self):
        """True when a step of Tc == 1 takes the fused one-launch-per-layer path (fused=True and fp32 operands)."""
        if self._layers is not None and self._prec != Fn._prec():
            return self.fused and Fn._prec() == 0  # (the next use refreshes)
        return self._fused_active

    @property
    def sparse_active(self):
        """True when a step of Tc == 1 takes the event-driven fused path (sparse=True and fused_active)."""
        return self.sparse and self.fused_active

    def _ensure(self):
        if self._layers is None or self._prec != Fn._prec():  # (the V pack is made for one operand mode)
            self.refresh()

    # ------------------------------------------------------------------ state
    @staticmethod
    def _entry(st, readout):
        """One layer's entry of a state list -> (u, w, s[, out]) tensors or None."""
        if readout:
            if torch.is_tensor(st):
                return st, None, None, None
            return st.get("u0", st.get("u")), None, None, st.get("out")
        if isinstance(st, dict):
            return st.get("u0", st.get("u")), st.get("w0", st.get("w")), st.get("s0", st.get("s")), None
        u, w, s = st
        return u, w, s, None

    def _load(self, states, rows):
        idx = self._rows(rows)
        for L, st in self._entries(states):
            u, w, s, out = self._entry(st, L.readout)
            self._put(L.u, u, "u", idx, L.H)
            hist = st.get("hist") if isinstance(st, dict) else None
            if L.D and hist is not None:
                n = self.batch_size if idx is None else len(idx)
                hist = torch.as_tensor(hist).to(self._dev)
                if tuple(hist.shape) != (n, L.D, L.K):
                    raise ValueError(f"StreamingSNN: hist has shape {tuple(hist.shape)}, expected ({n}, {L.D}, {L.K})")
                dst = self._hist(L, hist.dtype if idx is None else None)
                if idx is None:
                    dst.copy_(hist)
                else:
                    dst.index_copy_(0, idx, hist.to(dst.dtype))
            cur = st.get("i") if isinstance(st, dict) else None
            if L.syn is not None and cur is not None:
                self._put(L.i, cur, "i", idx, L.H)
            if L.readout:
                if out is not None:
                    self._put(L.out, out, "out", idx)
                steps = st.get("steps") if isinstance(st, dict) else None
                if steps is not None and L.steps is not None:
                    steps = torch.as_tensor(steps).to(device=self._dev, dtype=torch.int32).reshape(-1, 1)
                    if steps.shape[0] != (self.batch_size if idx is None else len(idx)):
                        raise ValueError(f"StreamingSNN: steps has {steps.shape[0]} rows")
                    if idx is None:
                        L.steps.copy_(steps)
                    else:
                        L.steps.index_copy_(0, idx, steps)
                continue
            if L.adaptive:
                self._put(L.w, w, "w", idx, L.H)
            self._put(L.s, s, "s", idx, L.H)
            L.binary = False  # drawn states are uniform noise; a caller's are whatever they are

    def reset(self, states=None, rows=None):
        """Start (the given rows of) the stream anew.  states=None draws u0, [w0,] s0 per hidden layer and the
        readout's u0 from torch's global CPU generator in exactly the order one SNN.forward draws them
        (`SNN.draw_states`): under the same torch.manual_seed the first chunk equals the beginning of net(x).
        states: a list with one entry per layer — (u0, w0, s0) or a dict with u0 / w0 / s0 (or u / w / s), for the
        readout a tensor or a dict with u0 — of batch_size rows, or of len(rows) rows.
        rows: reinitialise state, running output and step count of these rows only (independent streams that end at
        different times); the spike counters are per layer, not per row, and keep counting."""
        self._ensure()
        n = self.batch_size if rows is None else len(list(rows))
        if states is None:
            states = self.net.draw_states(n, self._dev)
            states.wait_ready()
        for L in self._layers:  # a delayed layer's history: no input seen yet (a `hist` entry of `states` replaces it)
            if L.hist is not None:
                if rows is None:
                    L.hist.zero_()
                else:
                    L.hist.index_fill_(0, self._rows(rows), 0)
            if L.i is not None:  # the synaptic current: none yet (an `i` entry of `states` replaces it)
                if rows is None:
                    L.i.zero_()
                else:
                    L.i.index_fill_(0, self._rows(rows), 0)
        self._load(states, rows)
        ro = self._layers[-1] if self._layers[-1].readout else None
        if rows is None:
            for L in self._layers:
                if not L.readout:
                    L.count.zero_()
            if ro is not None:
                ro.out.fill_(ro.out_init)
                if ro.steps is not None:
                    ro.steps.zero_()
        elif ro is not None:
            ro.out.index_fill_(0, self._rows(rows), ro.out_init)
            if ro.steps is not None:
                ro.steps.index_fill_(0, self._rows(rows), 0)
        self._restart(rows)

    def get_state(self):
        """A copy of the carried state: per hidden layer {"u", ["w",] "s"}, for the readout {"u", "out"} (unpadded);
        `out` is the accumulator as carried — in the mean readouts un-normalised, with the rows' step counts as "steps".
        A layer with axonal delays adds "hist" (B, max_delay, K): its last max_delay input steps, the newest last, in the
        dtype they travel in (bf16 for spikes and spike counts)."""
        self._ensure()
        res = []
        for L in self._layers:
            if L.readout:
                res.append({"u": L.u.clone(), "out": L.out.clone()})
                if L.steps is not None:
                    res[-1]["steps"] = L.steps.clone()
            else:
                d = {"u": L.u[:, :L.H].clone(), "s": L.s[:, :L.H].clone()}
                if L.adaptive:
                    d["w"] = L.w[:, :L.H].clone()
                res.append(d)
            if L.D:
                res[-1]["hist"] = self._hist(L, None).clone()
            if L.syn is not None:
                res[-1]["i"] = L.i.clone()
        return res

    def firing_rates(self):
        """Spikes per hidden unit / (B * steps_seen), the layers concatenated as SNN.forward concatenates them."""
        self._ensure()
        if self.steps_seen == 0:
            raise ValueError("StreamingSNN.firing_rates: no step seen yet")
        counts = [L.count[:L.H] for L in self._layers if not L.readout]
        c = torch.cat(counts) if len(counts) > 1 else counts[0]
        return c * (1.0 / float(self.batch_size * self.steps_seen))

    # ------------------------------------------------------------------ the chunk step
    def _hist(self, L, dtype):
        """The history buffer of a delayed layer, (B, D, K) zeros when first asked for; dtype None: as it is (fp32 if
        no chunk has been seen).  Another dtype than before (fp32 chunks after uint8 ones) converts what is carried."""
        if L.hist is None:
            L.hist = torch.zeros(self.batch_size, L.D, L.K, dtype=dtype or torch.float32, device=self._dev)
        elif dtype is not None and L.hist.dtype != dtype:
            L.hist = L.hist.to(dtype)
        return L.hist

    def _delayed(self, L, x, s16):
        """The chunk's input of a delayed layer, shifted (`sparch_delay_stream`; the history moves on): the network
        input x — its values, or the bf16 plane of a chunk of spike counts — or the previous layer's spike plane."""
        B = self.batch_size
        if s16 is not None:
            return x, Fn.delay_stream(s16, L.delay, L.D, self._hist(L, s16.dtype))
        tag = Fn.input_plane_of(x)
        if tag is None:
            return Fn.delay_stream(x, L.delay, L.D, self._hist(L, x.dtype)), None
        plane, flag = tag
        Tc, ld = x.shape[1], plane.shape[-1]
        store = (torch.empty if ld == L.K else torch.zeros)(B * Tc, ld, dtype=plane.dtype, device=self._dev)
        Fn.delay_stream(plane.view(B, Tc, ld)[:, :, :L.K], L.delay, L.D, self._hist(L, plane.dtype),
                        out=store.view(B, Tc, ld)[:, :, :L.K])
        y = Fn.spike_placeholder(B, Tc, L.K, self._dev).view(B, Tc, L.K)
        y._sparch_input_plane = (tuple(y.shape), store, flag)
        return y, None

    def _rec_drive(self, L):
        """s @ Vmasked for the state the next step starts from: the exact spike product on the bf16 plane once the
        state is binary (every chunk but the first after a reset), the dense six-term product on drawn states."""
        B = self.batch_size
        if L.binary:
            return Fn.gemm_nt(Fn.spike_placeholder(1, B, L.Hs, self._dev).view(B, L.Hs), L.vmask_t, spike_scale=1.0,
                              a16=L.s16)[0]
        if L.step_path:
            return Fn.gemm_nn(L.s, L.vmask)
        return Fn._gemm_small(L.s, L.vmask, nn=True)

    def _cell(self, L, Wx, Tc, want_fp32):
        """Wx (B*Tc, H) normalised projection (or raw + scale / shift) -> (s fp32 or None, s16), (B,Tc,H)."""
        B, H, Hs, dev = self.batch_size, L.H, L.Hs, self._dev
        if Hs != H:
            Wx = _pad_cols(Wx, Hs)
        s16 = torch.empty(B, Tc, Hs, dtype=torch.bfloat16, device=dev)
        s_out = torch.empty(B, Tc, Hs, dtype=torch.float32, device=dev) if want_fp32 else None
        k, p = KIND[L.kind], L.p
        if not L.recurrent:
            check(lib.sparch_cell_stream_fwd(k, B, 1, Tc, Hs, ptr(Wx), ptr(L.scale), ptr(L.shift), ptr(p["alpha"]),
                                             ptr(p.get("beta")), ptr(p.get("a")), ptr(p.get("b")), ptr(L.u), ptr(L.w),
                                             ptr(L.s), L.theta, 0.0, ptr(s_out), ptr(s16), ptr(L.count), Fn._stream()),
                  "sparch_cell_stream_fwd")
        elif L.step_path:
            for t in range(Tc):
                rec = self._rec_drive(L)
                check(lib.sparch_rec_cell_step_stream_fwd(k, B, 1, Tc, Hs, t, ptr(Wx), ptr(L.scale), ptr(L.shift),
                                                          ptr(p["alpha"]), ptr(p.get("beta")), ptr(p.get("a")),
                                                          ptr(p.get("b")), ptr(rec), ptr(L.u), ptr(L.w), ptr(L.s),
                                                          ptr(L.s16), L.theta, 0.0, ptr(s_out), ptr(s16), ptr(L.count),
                                                          Fn._stream()), "sparch_rec_cell_step_stream_fwd")
                L.binary = True
        else:
            rec0 = self._rec_drive(L)
            Fn._persistent(None, "sparch_rec_cell_stream_fwd",
                           (k, B, 1, Tc, Hs, ptr(Wx), ptr(L.scale), ptr(L.shift), ptr(p["alpha"]), ptr(p.get("beta")),
                            ptr(p.get("a")), ptr(p.get("b")), ptr(L.vpack), ptr(rec0), ptr(L.u), ptr(L.w), ptr(L.s),
                            ptr(L.s16), L.theta, 0.0, ptr(s_out), ptr(s16), ptr(L.count)),
                           lib.sparch_rec_chan_bytes(B, Tc, Hs), dev, Fn.rec_steps_per_launch(Tc), Fn._prec())
            L.binary = True
        if Hs != H:  # the next layer's operand at the layer's own width (the state stays padded)
            s16 = s16[..., :H].contiguous()
            s_out = None if s_out is None else s_out[..., :H].contiguous()
        return s_out, s16

    def _norm(self, L, Wx_raw):
        if L.norm == "layernorm":
            return Fn._Norm.forward("layernorm", Wx_raw, None, L.nw, L.nb, None, None, False, 1)[0]
        return Wx_raw  # batchnorm: folded into the cell's scale / shift

    def _body(self, x):
        """One chunk through every layer (eager launches, or the region a graph captures)."""
        B = self.batch_size
        Tc = x.shape[1]
        layers = self._layers
        s = s16 = None
        taps = []
        for i, L in enumerate(layers):
            if L.D:
                x, s16 = self._delayed(L, x, s16 if i else None)
            if i == 0:
                # the network input, as SpikingLayerFn.forward takes it: its bf16 plane when every value is bf16-exact
                # (binned spike counts are; decided on the device), the fp32 values otherwise
                inp = Fn._layer_input({"in_plane": Fn.input_plane_of(x)}, x)
                Wx_raw, _ = inp.project(L.W, L.Wb, False)
            else:  # the previous layer's spikes: their bf16 plane, beside a placeholder nobody reads
                inp = Fn._layer_input({"in_spike_scale": 1.0, "in_spike16": s16},
                                      Fn.spike_placeholder(B, Tc, L.K, self._dev))
                Wx_raw, _ = inp.project(L.W, L.Wb, False, b_planes=L.w_planes)
            Wx = self._norm(L, Wx_raw)
            if L.readout:
                if L.red != 0:
                    check(lib.sparch_readout_stream_fwd_red(B, Tc, L.H, ptr(Wx), ptr(L.scale), ptr(L.shift),
                                                            ptr(L.p["alpha"]), ptr(L.u), ptr(L.out), L.red, Fn._stream()),
                          "sparch_readout_stream_fwd_red")
                    if L.red_mean:  # accumulator / steps: the whole-sequence kernel's one division by (float)T_b
                        L.steps += Tc
                        return L.out / L.steps.to(torch.float32), taps
                    return L.out, taps
                check(lib.sparch_readout_stream_fwd(B, Tc, L.H, ptr(Wx), ptr(L.scale), ptr(L.shift), ptr(L.p["alpha"]),
                                                    ptr(L.u), ptr(L.out), Fn._stream()), "sparch_readout_stream_fwd")
                return L.out, taps
            if L.syn is not None:  # the synaptic current, carried in L.i and advanced by the chunk's steps
                Wx = Fn.synapse_stream(Wx.view(B, Tc, L.H), L.gamma, L.syn, L.i, scale=L.syn_scale,
                                       shift=L.syn_shift).view(B * Tc, L.H)
            s, s16 = self._cell(L, Wx, Tc, want_fp32=(i + 1 == len(layers)))
            taps.append(s16)
        return s, taps

    def _emit(self, taps):
        if self._spike_tap is not None:
            for i, t in enumerate(taps):
                self._spike_tap(i, t)

    def step(self, x_chunk, lengths=None, pack=False):
        """x_chunk (B,Tc,C) float32, uint8 spike counts, or a tagged count plane (`input_from_counts`, a spike
        encoder's output), on the device; any Tc >= 1."""
        if pack:
            raise ValueError("sparch_amd: pack=True is not supported by the streaming classes (StreamingSNN)")
        if lengths is not None:  # (a stream ends when its caller stops feeding it: DESIGN.md section 7)
            raise ValueError("sparch_amd: lengths are not supported by the streaming classes (StreamingSNN)")
        self._ensure()
        x = self._chunk(x_chunk)
        Tc = x.shape[1]
        # a chunk that is a tagged placeholder (input_from_counts, a spike encoder): its bf16 plane is the data and the
        # tensor has no values to read or copy, so it takes the chunk path's eager launches whatever its length
        tagged = Fn.input_plane_of(x) is not None
        if self._fused_active:
            if Tc == 1 and not tagged:
                with torch.no_grad():
                    out = self._fused_step(x)
                self.steps_seen += 1
                self.row_steps += 1
                return out
            if self.graph:
                self._primary_spikes()
        if x.dtype != torch.uint8 and not tagged:
            x = Fn._f32c(x)
        out = None
        with torch.no_grad():
            if self.graph and not tagged:
                out = self._graph_step(x, Tc)
            if out is None:
                xin = Fn.input_from_counts(x) if x.dtype == torch.uint8 else x
                out, taps = self._body(xin)
                self._emit(taps)
                if self._layers[-1].readout:
                    out = out.clone()  # (the buffer itself is the accumulator of the next step)
        self.steps_seen += Tc
        self.row_steps += Tc
        return out

    def _graph_step(self, x, Tc):
        """Replay (after capturing it once) the step for the first (B,Tc) seen; None = take the eager path: another
        Tc, a state that is not binary yet (the first chunk after a reset runs the dense boundary product), or the
        one eager pass that warms the kernels up before the capture."""
        if self._g_Tc is None:
            self._g_Tc = (Tc, x.dtype)
        if (Tc, x.dtype) != self._g_Tc or not all(L.binary for L in self._layers if L.recurrent):
            return None
        if self._g is None:
            if self._g_warm < 1:
                self._g_warm += 1
                return None
            g = {"x": x.clone(), "graph": torch.cuda.CUDAGraph()}
            torch.cuda.synchronize()
            with torch.cuda.graph(g["graph"]):
                xin = Fn.input_from_counts(g["x"]) if x.dtype == torch.uint8 else g["x"]
                out, g["taps"] = self._body(xin)
                g["out"] = out.clone()
            self._g = g
        self._g["x"].copy_(x, non_blocking=True)
        self._g["graph"].replay()
        self._g_replays += 1
        self._emit(self._g["taps"])
        return self._g["out"]

    # ------------------------------------------------------------------ the fused step (Tc == 1)
    def _state_key(self):
        return tuple(L.s.data_ptr() for L in self._layers if L.recurrent)

    def _primary_spikes(self):
        """Make the first spike buffer of every recurrent layer the current one (a copy after an odd number of fused
        steps): the captured chunk step of `_graph_step` holds the pointers it was captured with."""
        for L in self._layers:
            if L.recurrent and L.s is not L.s_first:
                L.s_alt.copy_(L.s)
                L.s16_alt.copy_(L.s16)
                L.s, L.s_alt, L.s16, L.s16_alt = L.s_alt, L.s, L.s16_alt, L.s16

    def _fused_launch(self, x, ldx):
        """The step's launches on the current buffers: one per layer.  x (B,1,K) fp32 or uint8 with unit stride
        along K and row stride ldx.  Returns the readout's accumulator, or the last layer's fresh spike buffer."""
        B = self.batch_size
        src, dt = x, int(x.dtype == torch.uint8)
        sparse = self.sparse_active
        for L in self._layers:
            if L.readout:
                if sparse:
                    check(lib.sparch_stream_step_sparse_readout(B, L.K, L.H, ptr(src), ldx, ptr(L.Wt), L.Wt.shape[1],
                                                                ptr(L.Wb), ptr(L.scale), ptr(L.shift), ptr(L.p["alpha"]),
                                                                ptr(L.u), ptr(L.out), Fn._stream()),
                          "sparch_stream_step_sparse_readout")
                    return L.out
                check(lib.sparch_stream_step_readout(B, L.K, L.H, ptr(src), ldx, ptr(L.W), ptr(L.Wb), ptr(L.scale),
                                                     ptr(L.shift), ptr(L.p["alpha"]), ptr(L.u), ptr(L.out),
                                                     Fn._stream()), "sparch_stream_step_readout")
                return L.out
            p = L.p
            s_out, s16_out = (L.s_alt, L.s16_alt) if L.recurrent else (L.s, None)
            if sparse:
                check(lib.sparch_stream_step_sparse_fwd(KIND[L.kind], B, L.K, L.H, L.Hs, dt, ptr(src), ldx, ptr(L.Wt),
                                                        L.Wt.shape[1], ptr(L.Wb), ptr(L.scale), ptr(L.shift),
                                                        ptr(p["alpha"]), ptr(p.get("beta")), ptr(p.get("a")),
                                                        ptr(p.get("b")), ptr(L.vmask) if L.recurrent else None, ptr(L.u),
                                                        ptr(L.w), ptr(L.s), ptr(s_out), ptr(s16_out), L.theta,
                                                        ptr(L.count), Fn._stream()), "sparch_stream_step_sparse_fwd")
                src, ldx, dt = s_out, L.Hs, 0
                continue
            check(lib.sparch_stream_step_fwd(KIND[L.kind], B, L.K, L.H, L.Hs, dt, ptr(src), ldx, ptr(L.W), ptr(L.Wb),
                                             ptr(L.scale), ptr(L.shift), ptr(p["alpha"]), ptr(p.get("beta")),
                                             ptr(p.get("a")), ptr(p.get("b")), ptr(L.vmask_t) if L.recurrent else None,
                                             ptr(L.u), ptr(L.w), ptr(L.s), ptr(s_out), ptr(s16_out), L.theta,
                                             ptr(L.count), Fn._stream()), "sparch_stream_step_fwd")
            src, ldx, dt = s_out, L.Hs, 0
        return src

    def _fused_swap(self):
        """Behind a fused step (launched or replayed): the written spike buffers become the current ones."""
        for L in self._layers:
            if L.readout:
                continue
            if L.recurrent:
                L.s, L.s_alt, L.s16, L.s16_alt = L.s_alt, L.s, L.s16_alt, L.s16
            L.binary = True

    def _fused_step(self, x):
        layers = self._layers
        if x.dtype not in (torch.uint8, torch.float32) or x.stride(2) != 1:
            x = x.contiguous() if x.dtype == torch.uint8 else Fn._f32c(x)
        ldx = max(int(x.stride(0)), layers[0].K)  # a (B,1,K) slice of a longer sequence is read where it lies
        ro = layers[-1].readout
        hidden = [L for L in layers if not L.readout]
        out = self._replayed_step(self._fg, x) if self.graph else None
        if out is None:
            out = self._fused_launch(x, ldx)
            out = out.clone() if ro else out[:, :hidden[-1].H].unsqueeze(1).clone()
        self._fused_swap()
        if self._spike_tap is not None:
            for i, L in enumerate(hidden):
                self._spike_tap(i, L.s[:, :L.H].unsqueeze(1))
        return out

    def _static_step(self, x):
        """The three-launch chain on the static input, as a graph captures it."""
        out, last = self._fused_launch(x, self._layers[0].K), self._layers[-1]
        return out if last.readout else out[:, :last.H].unsqueeze(1)


# ---------------------------------------------------------------------------------------- raw audio
FBANK_WINDOW, FBANK_SHIFT = 400, 160  # 25 ms frames every 10 ms at 16 kHz (csrc/fbank_frame.h)


def fbank_stream_plan(tail, n_new):
    """Frame arithmetic of a streamed Kaldi filterbank with snip_edges=True (pure host): with `tail` unconsumed
    samples kept and `n_new` arriving, returns (frames that are complete now, samples to keep afterwards).  Frame j
    covers samples [160 j, 160 j + 400) of the stream and depends on nothing else, so the frames of tail + chunk are
    the stream's next frames; what is kept starts at the first frame that is not complete yet: at most 399 samples,
    and 240 .. 399 once a frame has been made."""
    total = int(tail) + int(n_new)
    if total < FBANK_WINDOW:
        return 0, total
    frames = 1 + (total - FBANK_WINDOW) // FBANK_SHIFT
    return frames, total - frames * FBANK_SHIFT


class StreamingFbank:
    """push(wave_chunk (B,n)) -> (B, new_frames, num_mel_bins): the log-mel frames that became complete, from the
    library's fbank kernel run on the kept tail + the chunk (per-frame DC removal and pre-emphasis are per frame, so
    they equal the frames of the whole clip bit for bit)."""

    def __init__(self, batch_size, num_mel_bins=40):
        self.batch_size, self.num_mel_bins = int(batch_size), int(num_mel_bins)
        self.tail = None
        self.frames_seen = 0

    def reset(self):
        self.tail, self.frames_seen = None, 0

    def push(self, wave_chunk):
        Fn._require_device(wave_chunk, "waveform")
        w = Fn._f32c(wave_chunk)
        if w.ndim != 2 or w.shape[0] != self.batch_size:
            raise ValueError(f"StreamingFbank.push: a ({self.batch_size}, n) chunk, got {tuple(w.shape)}")
        buf = w if self.tail is None else torch.cat([self.tail, w], dim=1)
        frames, keep = fbank_stream_plan(0 if self.tail is None else self.tail.shape[1], w.shape[1])
        if frames == 0:
            self.tail = buf.clone() if buf is w else buf  # never keep the caller's own buffer
            return torch.empty(self.batch_size, 0, self.num_mel_bins, dtype=torch.float32, device=w.device)
        out = Fn.fbank(buf, self.num_mel_bins)
        self.tail = buf[:, buf.shape[1] - keep:].clone()
        self.frames_seen += frames
        return out
