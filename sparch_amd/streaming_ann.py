"""
Streaming inference for the non-spiking baselines: a trained `sparch_amd.anns.ANN` (MLP, RNN, LiGRU, GRU) answers a
stream step by step, carrying every recurrent layer's state.

    st = StreamingANN(net, batch_size)          # net.eval(), unidirectional, fp32 operands
    st.reset()                                  # y = 0, as the reference starts (anns.py:331, 452, 584)
    out = st.step(x_chunk)                      # (B,Tc,C), any Tc >= 1 -> norm(W sum_t softmax(y_t)) (B,classes)

What is carried per recurrent layer is y after the last step, for the readout the running sum `acc` of the softmaxes:
a step of the cells needs nothing else.  Every chunk is served as Tc fused steps (csrc/streamann.hip), each reading
x[:, t] where it lies: `sparch_ann_stream_step` does the projection(s), the eval BatchNorm affine, y V^T and the cell of
a hidden layer in one launch (two for a GRU layer), `sparch_ann_stream_readout` adds softmax(y_t) to the accumulator
— one sequential sum over t — and returns the network's answer as if the sequence ended at this step.  The arithmetic
of a step does not know where a chunk ends, so any chunking of a stream gives the same bits.  Every workgroup of a
recurrent layer reads all of the previous y, so those layers keep y twice and the host swaps which copy is current
after each step.  LayerNorm is a row statistic across the workgroups of a step: such a layer's projection(s) go through
the library's GEMM and `sparch_layernorm_fwd`, and the step kernel takes them ready-made.

There is no whole-chunk kernel with state for the baselines and no bf16 operand mode of the fused step, hence the
refusal of compute dtype bf16.
"""
import ctypes

import torch

from . import functional as Fn
from ._capi import check, lib, ptr
from .streaming import _Layer, _ParityGraphs, _Stream

CELL = {"MLP": 0, "RNN": 1, "LiGRU": 2, "GRU": 3}          # SPARCH_CELL_*
RO_NORM = {"none": 0, "batchnorm": 1, "layernorm": 2}      # SPARCH_RO_NORM_*
_SLOT = {"": 0, "z": 1, "r": 2}                            # the gate slots of sparch_ann_stream_step
_Slots = ctypes.c_void_p * 3


def _slots(tensors):
    """Three tensors (or None) -> the host array of device pointers the entry point takes (None: all NULL)."""
    if all(t is None for t in tensors):
        return None
    return _Slots(*[ptr(t) for t in tensors])


class StreamingANN(_Stream):
    """Step-by-step forward of a `sparch_amd.anns.ANN` in eval mode with carried state.

    step(x_chunk) returns, with a readout layer, the readout's output (B,classes) after all steps seen so far,
    without one the last layer's outputs of the chunk (B,Tc,H); with graph=True and Tc == 1 a static tensor that the
    next step overwrites.  Nothing here synchronises with the device."""

    def __init__(self, net, batch_size, graph=False):
        if getattr(net, "is_snn", False):
            raise ValueError("StreamingANN: a sparch_amd.anns.ANN (a spiking network streams through StreamingSNN)")
        if not hasattr(net, "ann"):
            raise ValueError("StreamingANN: a sparch_amd.anns.ANN")
        super().__init__(net, batch_size, graph)
        self._require_fp32()
        self._parity = 0          # which copy of the recurrent states is current
        self._g = _ParityGraphs()  # graph=True: keyed by the parity

    @staticmethod
    def _require_fp32():
        if Fn._prec() != 0:
            raise ValueError("StreamingANN: compute dtype bf16 — the fused step is fp32 FMA only and the baselines have "
                             "no chunk path to fall back to; set_compute_dtype('fp32')")

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
        zeros = lambda n: torch.zeros(B, n, dtype=torch.float32, device=dev)  # noqa: E731

        def fold(L, norm):
            """The eval form of one normalisation: (scale, shift) of BatchNorm's running statistics, or (gamma, beta)."""
            if L.norm == "batchnorm":
                return self._bn_fold(L.H, norm)
            if L.norm == "layernorm":
                return Fn._f32c(norm.weight.detach()), Fn._f32c(norm.bias.detach())
            return None, None

        with torch.no_grad():
            for i, mod in enumerate(net.ann):
                L = _Layer()
                L.readout = bool(net.use_readout_layer and i == last)
                L.norm = mod.normalization if mod.normalize else "none"
                L.K = mod.input_size
                if L.readout:
                    L.H = mod.output_size
                    L.W = Fn._f32c(mod.W.weight.detach())
                    L.Wb = None if mod.W.bias is None else Fn._f32c(mod.W.bias.detach())
                    L.p0, L.p1 = fold(L, mod.norm if mod.normalize else None)
                    L.acc = old[i].acc if old is not None else zeros(L.K)
                    L.out = old[i].out if old is not None else zeros(L.H)
                    layers.append(L)
                    continue
                L.kind, L.H = net.ann_type, mod.hidden_size
                L.recurrent = L.kind != "MLP"
                L.act = Fn.ACT_KIND["sigmoid"]  # (the MLP's and the RNN's; the gated cells have their own)
                W, Wb, n0, n1, V = ([None] * 3 for _ in range(5))
                for g in mod.GATES:
                    s = _SLOT[g]
                    lin = getattr(mod, "W" + g)
                    W[s] = Fn._f32c(lin.weight.detach())
                    Wb[s] = None if lin.bias is None else Fn._f32c(lin.bias.detach())
                    n0[s], n1[s] = fold(L, getattr(mod, "norm" + g) if mod.normalize else None)
                    if L.recurrent:
                        V[s] = Fn._f32c(getattr(mod, "V" + g).weight.detach())
                L.gates = sorted(_SLOT[g] for g in mod.GATES)
                L.W, L.Wb, L.n0, L.n1, L.V = W, Wb, n0, n1, V        # (the arrays below point into these)
                L.W_p, L.Wb_p, L.V_p = _slots(W), _slots(Wb), _slots(V)
                bn = L.norm == "batchnorm"
                L.scale_p, L.shift_p = (_slots(n0), _slots(n1)) if bn else (None, None)
                # state buffers: kept across refresh()
                if old is not None:
                    L.y, L.y_alt, L.z, L.ry = old[i].y, old[i].y_alt, old[i].z, old[i].ry
                else:
                    L.y = zeros(L.H)
                    L.y_alt = zeros(L.H) if L.recurrent else None     # the other copy: a step reads y, writes y_alt
                    L.z, L.ry = (zeros(L.H), zeros(L.H)) if L.kind == "GRU" else (None, None)
                layers.append(L)
        self._layers = layers
        self._g = _ParityGraphs()  # a captured step holds the old operands

    def _ensure(self):
        self._require_fp32()
        if self._layers is None:
            self.refresh()

    # ------------------------------------------------------------------ state
    def _load(self, states, idx):
        for L, st in self._entries(states):
            if not L.readout and not L.recurrent:
                continue  # an MLP layer carries nothing
            key = "acc" if L.readout else "y"
            self._put(L.acc if L.readout else L.y, st.get(key) if isinstance(st, dict) else st, key, idx)

    def reset(self, states=None, rows=None):
        """Start (the given rows of) the stream anew: y = 0 and an empty accumulator, as the reference's forward
        starts, or `states` in the format of get_state() with batch_size rows (or len(rows) rows).
        rows: reinitialise state, accumulator and step count of these rows only (independent streams that end at
        different times)."""
        self._ensure()
        idx = self._rows(rows)
        for L in self._layers:
            for buf in ((L.acc, L.out) if L.readout else (L.y,)):
                if idx is None:
                    buf.zero_()
                else:
                    buf.index_fill_(0, idx, 0.0)
        if states is not None:
            self._load(states, idx)
        self._restart(rows)

    def get_state(self):
        """A copy of the carried state: per hidden layer {"y"} ({} for an MLP layer), for the readout {"acc"}."""
        self._ensure()
        res = []
        for L in self._layers:
            if L.readout:
                res.append({"acc": L.acc.clone()})
            else:
                res.append({"y": L.y.clone()} if L.recurrent else {})
        return res

    # ------------------------------------------------------------------ one step
    def _project_ln(self, L, src):
        """LayerNorm layers: norm(src W?^T + bias) per gate through the GEMM and sparch_layernorm_fwd -> `pre` slots."""
        pre = [None] * 3
        for s in L.gates:
            raw, _ = Fn.gemm_nt(src, L.W[s], L.Wb[s])
            pre[s] = Fn._Norm.forward("layernorm", raw, None, L.n0[s], L.n1[s], None, None, False, 1)[0]
        return pre

    def _launch(self, x):
        """The step's launches on the current buffers.  x (B,K) fp32 with unit stride along K.  Returns the readout's
        output, or the last layer's fresh y."""
        B = self.batch_size
        src = x
        for L in self._layers:
            ldx = max(int(src.stride(0)), L.K)
            if L.readout:
                check(lib.sparch_ann_stream_readout(B, L.K, L.H, ptr(src), ldx, ptr(L.acc), ptr(L.W), ptr(L.Wb),
                                                    RO_NORM[L.norm], ptr(L.p0), ptr(L.p1), Fn.NORM_EPS, ptr(L.out),
                                                    Fn._stream()), "sparch_ann_stream_readout")
                return L.out
            pre = self._project_ln(L, src) if L.norm == "layernorm" else None
            xin, W_p, Wb_p = (None, None, None) if pre is not None else (src, L.W_p, L.Wb_p)
            dst = L.y_alt if L.recurrent else L.y
            for phase in ((1, 2) if L.kind == "GRU" else (0,)):
                check(lib.sparch_ann_stream_step(CELL[L.kind], phase, L.act, B, L.K, L.H, L.H, ptr(xin), ldx, W_p, Wb_p,
                                                 L.scale_p, L.shift_p, _slots(pre) if pre is not None else None, L.V_p,
                                                 ptr(L.y) if L.recurrent else None, None if phase == 1 else ptr(dst),
                                                 ptr(L.z), ptr(L.ry), Fn._stream()), "sparch_ann_stream_step")
            src = dst
        return src

    def _swap(self):
        """Behind a step (launched or replayed): the written copies of the recurrent states become the current ones."""
        for L in self._layers:
            if not L.readout and L.recurrent:
                L.y, L.y_alt = L.y_alt, L.y
        self._parity ^= 1

    def step(self, x_chunk, lengths=None, pack=False):
        """x_chunk (B,Tc,C) float32 (or uint8 counts, converted here) on the device, 4-D when net.reshape; Tc >= 1."""
        if pack:
            raise ValueError("sparch_amd: pack=True is not supported by the streaming classes (StreamingANN)")
        if lengths is not None:  # 
            raise ValueError("sparch_amd: lengths are not supported by the streaming classes (StreamingANN)")
        self._ensure()
        x = self._chunk(x_chunk)
        if x.dtype != torch.float32 or x.stride(2) != 1:
            x = Fn._f32c(x)
        Tc = x.shape[1]
        ro = self._layers[-1].readout
        with torch.no_grad():
            out = self._replayed_step(self._g, x) if (self.graph and Tc == 1) else None
            if out is not None:
                self._swap()
            else:
                outs = None if ro else torch.empty(self.batch_size, Tc, self._layers[-1].H, dtype=torch.float32,
                                                   device=self._dev)
                for t in range(Tc):  # x[:, t] is read where it lies: the row stride is that of the chunk
                    y = self._launch(x[:, t])
                    self._swap()
                    if not ro:
                        outs[:, t].copy_(y)
                out = y.clone() if ro else outs
        self.steps_seen += Tc
        self.row_steps += Tc
        return out

    def _state_key(self):
        return self._parity

    def _static_step(self, x):
        """The chain of launches on the static input, as a graph captures it."""
        y = self._launch(x[:, 0])
        return y if self._layers[-1].readout else y.unsqueeze(1)
