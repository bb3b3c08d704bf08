"""
`Experiment` — the trainer behind run_exp.py, API-compatible with the reference's
sparch/exp.py (Experiment(args) / .forward(), exp.py:36-147): experiment folders and naming
(149-189), logging (191-212), model construction (291-339), Adam + ReduceLROnPlateau + cross-entropy
(88-100), train / valid / test epoch loops with the same log lines (341-518), best-model
checkpointing as a whole-module pickle (456-463, 126-133).

The training step itself (exp.py:352-382) runs on the MI355X path: `sparch_amd.SNN` on a HIP device.
What this build adds, not replaces:
  * --synthetic 1: batches of the dataset's shape generated on the fly (no dataset files needed);
    without it SHD/SSC go through sparch_amd.dataloaders.spiking_datasets (h5py event lists binned on the
    device; with SPARCH_EVENTS=resident the whole split stays on the device and each batch is one kernel;
    --use_augm 1 with SPARCH_EVENTS_AUGMENT=SPEC then augments the training events inside that kernel)
    and HD/SC through sparch_amd.dataloaders.nonspiking_datasets (audio files decoded on the host);
  * hd / sc inputs are raw waveforms turned into 40-bin log-mel features ON THE DEVICE (the reference calls
    torchaudio's kaldi.fbank per clip on the CPU, nonspiking_datasets.py:96, 194): by the file loaders' collate
    function (`sparch_amd.fbank_padded`: clips of different lengths, zero-padded features as pad_sequence pads
    them), and for synthetic one-second waves by the trainer (`sparch_amd.fbank`);
  * data parallelism when launched under torch.distributed.run: per-rank batch shard, per-layer
    gradient all-reduce over RCCL (`sparch_amd.dp.GradAllReducer`); rank 0 logs and checkpoints.
"""
import errno
import logging
import os
import time
from datetime import timedelta

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.optim.lr_scheduler import ReduceLROnPlateau

from . import dp, optim
from . import functional as Fn
from .functional import check_status, fbank
from .parsers import print_model_options, print_training_options
from .anns import ANN
from .encoders import SpikeEncoder, _mix64, parse_encode
from .snns import SNN, parse_surrogate

logger = logging.getLogger(__name__)

_SPIKING_SETS = {"shd": 20, "ssc": 35}
_AUDIO_SETS = {"hd": 20, "sc": 35}


class _SyntheticLoader:
    """Yields (x, xlens, y) like the reference's collate functions (spiking_datasets.py:80-87,
    nonspiking_datasets.py:105-112): spiking sets give (B, T, 700) float spike counts, audio sets give
    (B, 16000) waveforms in [-1, 1] that the trainer converts to (B, 98, 40) log-mel on the device."""

    def __init__(self, kind, batch_size, n_batches, n_classes, seq_len, seed):
        self.kind, self.batch_size, self.n_batches = kind, batch_size, n_batches
        self.n_classes, self.seq_len, self.seed = n_classes, seq_len, seed
        self._pool = None

    def __len__(self):
        return self.n_batches

    def __iter__(self):
        # the batches are generated ONCE (45 M random numbers per headline batch: 0.2 s of host time each, thirty
        # times a 7 ms training step) and served from pinned host memory every epoch — like a dataset that sits in
        # RAM; each epoch still moves every batch over PCIe
        if self._pool is None:
            self._pool = list(self._generate())
        return iter(self._pool)

    def _generate(self):
        g = torch.Generator().manual_seed(self.seed)
        pin = torch.cuda.is_available()
        for _ in range(self.n_batches):
            y = torch.randint(0, self.n_classes, (self.batch_size,), generator=g)
            if self.kind == "spiking":
                # class-dependent input: a band of 700 // n_classes channels fires at 0.25 instead of 0.04,
                # so that a run on synthetic data has something to learn (labels are not independent of x)
                band = 700 // self.n_classes
                ch = torch.arange(700)[None, :]
                hot = (ch >= y[:, None] * band) & (ch < (y[:, None] + 1) * band)
                rate = torch.where(hot, torch.tensor(0.25), torch.tensor(0.04))[:, None, :]
                # one byte per element: binned spike counts are small integers (spiking_datasets.py:71-78); the
                # trainer expands them on the device (functional.input_from_counts) instead of moving 4x the bytes
                # over PCIe every step as the reference does (exp.py:355-356)
                x = (torch.rand(self.batch_size, self.seq_len, 700, generator=g) < rate).to(torch.uint8)
                xlens = torch.full((self.batch_size,), self.seq_len)
            else:
                t = torch.arange(16000) / 16000.0
                tone = torch.sin(2 * np.pi * (200.0 + 40.0 * y[:, None].float()) * t[None])
                x = 0.1 * (torch.rand(self.batch_size, 16000, generator=g) * 2 - 1) + 0.3 * tone
                xlens = torch.full((self.batch_size,), 98)
            if pin:
                x = x.pin_memory()
            yield x, xlens, y


def parse_lengths_mode(value):
    """SPARCH_LENGTHS: unset or empty -> False (the lengths are dropped, the reference's behaviour), "mask" -> True,
    "pack" -> "pack" (the lengths go with the batch and the padded steps are skipped: SNN.forward(..., pack=True));
    anything else is refused."""
    if value is None or value == "":
        return False
    if value == "mask":
        return True
    if value == "pack":
        return "pack"
    raise ValueError(f"SPARCH_LENGTHS={value!r}: the values are 'mask' and 'pack' (unset: clips run to the batch's "
                     "longest one)")


def parse_clip_grad(value):
    """SPARCH_CLIP_GRAD: unset or empty -> None (no clipping, no new call); a positive number or "inf" (measure the
    gradient norm and skip non-finite steps without scaling) -> that float; anything else is refused."""
    if value is None or value.strip() == "":
        return None
    try:
        c = float(value)
    except ValueError:
        c = float("nan")
    if not c > 0:
        raise ValueError(f"SPARCH_CLIP_GRAD={value!r}: a positive number or 'inf' (the cap on the global gradient norm)")
    return c


def parse_per_step_loss(value):
    """SPARCH_PER_STEP_LOSS=w[:t0]: unset or empty -> None; else (w, t0) with the weight w a finite number > 0 and the
    first step t0 an integer >= 0 (default 0); anything else is refused."""
    if value is None or value.strip() == "":
        return None
    head, sep, tail = value.strip().partition(":")
    try:
        w = float(head)
        t0 = int(tail) if sep else 0
    except ValueError:
        w, t0 = float("nan"), 0
    if not (0 < w < float("inf")) or t0 < 0:
        raise ValueError(f"SPARCH_PER_STEP_LOSS={value!r}: w[:t0] with a weight w > 0 and a first step t0 >= 0 "
                         "(an integer; default 0)")
    return w, t0


def parse_readout(value):
    """SPARCH_READOUT=<mode>: unset or empty -> None (the reference's softmax-sum, nothing changes); else one of
    functional.READOUT_MODES; anything else is refused."""
    if value is None or value.strip() == "":
        return None
    name = value.strip()
    if name not in Fn.READOUT_MODES:
        raise ValueError(f"SPARCH_READOUT={value!r}: the values are {', '.join(Fn.READOUT_MODES)} (unset: softmax_sum)")
    return name


def parse_tbptt(value):
    """SPARCH_TBPTT=K: unset or empty -> None (whole-sequence training, nothing changes); else the chunk length K, an
    integer >= 1 (truncated BPTT: SNN.forward(state=..., return_state=True)); anything else is refused."""
    if value is None or value.strip() == "":
        return None
    try:
        k = int(value.strip())
    except ValueError:
        k = 0
    if k < 1:
        raise ValueError(f"SPARCH_TBPTT={value!r}: the chunk length in time steps, an integer >= 1 (unset: every batch is "
                         "one whole-sequence step)")
    return k


def parse_delays(value):
    """SPARCH_DELAYS=D[:zero|uniform][:fixed][:hidden]: unset or empty -> None (no delays, nothing changes); else the
    SNN arguments {"max_delay": D (an integer in [1, 255]), "delay_init": "zero" (default) or "uniform", "learn_delays":
    False with `fixed`, "delay_layers": "hidden" with `hidden` (default "all")}; the options in any order, each at most
    once; anything else is refused."""
    if value is None or value.strip() == "":
        return None
    head, *opts = [part.strip() for part in value.strip().split(":")]
    try:
        d = int(head)
    except ValueError:
        d = 0
    res = {"max_delay": d, "delay_init": None, "learn_delays": True, "delay_layers": "all"}
    ok = 1 <= d <= Fn.MAX_DELAY_CAP
    for opt in opts:
        if opt in ("zero", "uniform") and res["delay_init"] is None:
            res["delay_init"] = opt
        elif opt == "fixed" and res["learn_delays"]:
            res["learn_delays"] = False
        elif opt == "hidden" and res["delay_layers"] == "all":
            res["delay_layers"] = "hidden"
        else:
            ok = False
    if not ok:
        raise ValueError(f"SPARCH_DELAYS={value!r}: D[:zero|uniform][:fixed][:hidden] with the largest delay D an integer "
                         f"in [1, {Fn.MAX_DELAY_CAP}] time steps (unset: no delays)")
    res["delay_init"] = res["delay_init"] or "zero"
    return res


def parse_synapse(value):
    """SPARCH_SYNAPSE=lo:hi[:lo|uniform][:fixed][:hidden]: unset or empty -> None (no synapse, nothing changes); else the
    SNN arguments {"synapse": (lo, hi) with 0 <= lo <= hi < 1, "syn_init": "uniform" (default) or "lo", "learn_synapse":
    False with `fixed`, "synapse_layers": "hidden" with `hidden` (default "all")}; the options in any order, each at most
    once; anything else is refused."""
    if value is None or value.strip() == "":
        return None
    parts = [part.strip() for part in value.strip().split(":")]
    ok = len(parts) >= 2
    lo = hi = float("nan")
    if ok:
        try:
            lo, hi = float(parts[0]), float(parts[1])
        except ValueError:
            ok = False
    ok = ok and 0.0 <= lo <= hi < 1.0
    res = {"synapse": (lo, hi), "syn_init": None, "learn_synapse": True, "synapse_layers": "all"}
    for opt in parts[2:]:
        if opt in ("lo", "uniform") and res["syn_init"] is None:
            res["syn_init"] = opt
        elif opt == "fixed" and res["learn_synapse"]:
            res["learn_synapse"] = False
        elif opt == "hidden" and res["synapse_layers"] == "all":
            res["synapse_layers"] = "hidden"
        else:
            ok = False
    if not ok:
        raise ValueError(f"SPARCH_SYNAPSE={value!r}: lo:hi[:lo|uniform][:fixed][:hidden] with the limits of the synaptic "
                         "decay 0 <= lo <= hi < 1 (unset: no synapse)")
    res["syn_init"] = res["syn_init"] or "uniform"
    return res


def check_encode_model(net, encoder):
    """SPARCH_ENCODE with a given network (a loaded one included): a spiking network whose first layer is as wide as
    the encoder's output — refused before the first kernel otherwise."""
    if not getattr(net, "is_snn", False):
        raise ValueError(f"sparch_amd: SPARCH_ENCODE needs a spiking model (got {type(net).__name__})")
    width = int(net.snn[0].input_size)
    if width != encoder.out_features:
        raise ValueError(f"sparch_amd: SPARCH_ENCODE: the {encoder.code} code gives {encoder.out_features} input features, "
                         f"the model's first layer takes {width}")


def _step_lengths(seq, lengths):
    B, T = seq.shape[0], seq.shape[1]
    if lengths is None:
        return torch.full((B,), T, dtype=torch.long, device=seq.device)
    return torch.as_tensor(lengths).to(device=seq.device, dtype=torch.long)


def per_step_nll(seq_sum, y, lengths=None, t0=0):
    """Loss on early decisions.  seq_sum (B,T,C): the readout's running sum (SNN.forward(..., per_step="sum")), y (B,)
    labels, lengths (B,) or None (every clip has T steps).  seq_sum[b,t] / (t + 1) is a distribution over the classes
    (a mean of softmaxes); returns the mean, over the pairs (b, t) with t0 <= t < lengths[b], of its negative log at
    the label — 0 if there is no such pair."""
    B, T, _ = seq_sum.shape
    steps = torch.arange(T, device=seq_sum.device)
    at_label = seq_sum.gather(2, y.view(B, 1, 1).expand(B, T, 1)).squeeze(2) / (steps + 1).to(seq_sum.dtype)
    valid = (steps[None, :] >= t0) & (steps[None, :] < _step_lengths(seq_sum, lengths)[:, None])
    nll = -torch.log(torch.where(valid, at_label, torch.ones_like(at_label)).clamp_min(torch.finfo(seq_sum.dtype).tiny))
    return nll.sum() / valid.sum().clamp_min(1).to(seq_sum.dtype)


def decision_steps(seq_sum, y, lengths=None):
    """(B,) integers: per clip the earliest step t from which argmax seq_sum[b, t'] is the label for ALL t' with
    t <= t' < lengths[b]; a clip whose last step is still wrong never settles and counts at lengths[b]."""
    T = seq_sum.shape[1]
    steps = torch.arange(T, device=seq_sum.device)
    valid = steps[None, :] < _step_lengths(seq_sum, lengths)[:, None]
    wrong = (seq_sum.argmax(dim=2) != y[:, None]) & valid
    return (wrong.long() * (steps + 1)[None, :]).amax(dim=1)  # one past the last wrong step (0: right from the start)


class Experiment:
    """Training / testing of spiking networks on the four speech-command datasets."""

    def __init__(self, args):
        for k, v in vars(args).items():
            setattr(self, k, v)
        self.synthetic = getattr(args, "synthetic", False)
        self.synthetic_batches = getattr(args, "synthetic_batches", 8)
        self.seq_len = getattr(args, "seq_len", 100)
        self.sync_bn = getattr(args, "sync_bn", False)
        self.compute_dtype = getattr(args, "compute_dtype", "fp32")

        # SPARCH_SURROGATE=name[:scale]: the spiking layers' surrogate gradient (snns.resolve_surrogate).  Parsed once,
        # here, so that a malformed value is refused before folders, data or device are touched.
        spec = os.environ.get("SPARCH_SURROGATE", "")
        self.surrogate = parse_surrogate(spec) if spec.strip() else None
        # SPARCH_CLIP_GRAD=<positive float>|inf: clip the gradients by their global norm inside the optimizer step
        # (optim.Adam(max_grad_norm=...)); refused here for the same reason
        self.clip_grad = parse_clip_grad(os.environ.get("SPARCH_CLIP_GRAD"))

        # SPARCH_LENGTHS=mask: train, validation and test pass each batch's clip lengths to the network (ragged
        # batches, SNN.forward); unset: every clip runs to the batch's longest one, as in the reference
        # SPARCH_LENGTHS=pack: the same, in the packed layout (the padded steps are skipped instead of masked)
        self.lengths_mode = {False: None, True: "mask", "pack": "pack"}[parse_lengths_mode(os.environ.get("SPARCH_LENGTHS"))]
        mode = self.lengths_mode
        if mode and self.sync_bn:
            raise ValueError(f"sparch_amd: SPARCH_LENGTHS={mode} with --sync_bn is not supported")
        if mode and self.model_type not in ["LIF", "adLIF", "RLIF", "RadLIF"] and not self.use_pretrained_model:
            raise ValueError(f"sparch_amd: SPARCH_LENGTHS={mode} needs a spiking model (got {self.model_type})")
        if mode == "pack" and not self.use_pretrained_model:
            if getattr(args, "bidirectional", False):
                raise ValueError("sparch_amd: SPARCH_LENGTHS=pack with --bidirectional is not supported")
            if self.model_type in ["RLIF", "RadLIF"] and Fn.rec_steps_per_launch(2) < 2:
                raise ValueError("sparch_amd: SPARCH_LENGTHS=pack in the degraded step mode (one recurrent launch per time "
                                 "step, SPARCH_REC_STEPS_PER_LAUNCH=1) is not supported (use SPARCH_LENGTHS=mask)")
            if self.model_type in ["RLIF", "RadLIF"] and Fn.rec_step_path(getattr(args, "nb_hiddens", 0)):
                raise ValueError(f"sparch_amd: SPARCH_LENGTHS=pack with recurrent layers above 1024 hidden units (got "
                                 f"{args.nb_hiddens}) is not supported (use SPARCH_LENGTHS=mask)")

        # SPARCH_PER_STEP_LOSS=w[:t0]: the training loss gains w x per_step_nll on the readout's running sum from step
        # t0 on, and validation / test log the mean decision step ("Per-step readout")
        self.per_step_loss = parse_per_step_loss(os.environ.get("SPARCH_PER_STEP_LOSS"))
        if self.per_step_loss is not None:
            if mode == "pack":
                raise ValueError("sparch_amd: SPARCH_PER_STEP_LOSS with SPARCH_LENGTHS=pack is not supported (the per-step "
                                 "readout has no packed form; use SPARCH_LENGTHS=mask)")
            if self.model_type not in ["LIF", "adLIF", "RLIF", "RadLIF"] and not self.use_pretrained_model:
                raise ValueError(f"sparch_amd: SPARCH_PER_STEP_LOSS needs a spiking model (got {self.model_type})")

        # SPARCH_READOUT=<mode>: the readout layer's reduction over time (SNN(readout=...); DESIGN.md section 6,
        # "Selectable readout").  The loss stays cross-entropy on the network's output.
        self.readout = parse_readout(os.environ.get("SPARCH_READOUT"))
        if self.readout not in (None, "softmax_sum"):
            if self.per_step_loss is not None:
                raise ValueError(f"sparch_amd: SPARCH_READOUT={self.readout} with SPARCH_PER_STEP_LOSS is not supported "
                                 "(the per-step readout is the softmax-sum's)")
            if self.model_type not in ["LIF", "adLIF", "RLIF", "RadLIF"]:
                raise ValueError(f"sparch_amd: SPARCH_READOUT needs a spiking model (got {self.model_type})")

        # SPARCH_TBPTT=K: classic truncated BPTT — every training batch is cut into ceil(T / K) chunks, each started from
        # the detached state the one before ended in, with one optimizer step per chunk ("Stateful
        # training").  Validation and test are unchanged.
        self.tbptt = parse_tbptt(os.environ.get("SPARCH_TBPTT"))
        self._tbptt_steps = 0  # optimizer steps taken by chunks (logged per epoch)
        if self.tbptt is not None:
            for on, what in ((mode, f"SPARCH_LENGTHS={mode}"), (self.per_step_loss is not None, "SPARCH_PER_STEP_LOSS"),
                             (self.readout not in (None, "softmax_sum"), f"SPARCH_READOUT={self.readout}"),
                             (getattr(args, "bidirectional", False), "--bidirectional"), (self.sync_bn, "--sync_bn"),
                             (self.compute_dtype == "bf16", "--compute_dtype bf16")):
                if on:
                    raise ValueError(f"sparch_amd: SPARCH_TBPTT with {what} is not supported")
            if self.model_type not in ["LIF", "adLIF", "RLIF", "RadLIF"]:
                raise ValueError(f"sparch_amd: SPARCH_TBPTT needs a spiking model (got {self.model_type})")

        # SPARCH_DELAYS=D[:zero|uniform][:fixed][:hidden]: a learnable (or fixed) axonal delay of at most D steps per
        # input feature of every layer (or of every layer but the first) — SNN(max_delay=...); DESIGN.md section 6,
        # "Axonal delays".  Every epoch logs each delayed layer's mean and largest delay.
        self.delays = parse_delays(os.environ.get("SPARCH_DELAYS"))
        if self.delays is not None:
            if self.model_type not in ["LIF", "adLIF", "RLIF", "RadLIF"]:
                raise ValueError(f"sparch_amd: SPARCH_DELAYS needs a spiking model (got {self.model_type})")
            if self.tbptt is not None:
                raise ValueError("sparch_amd: SPARCH_DELAYS with SPARCH_TBPTT is not supported (the delayed input is "
                                 "not carried across chunks)")

        # SPARCH_SYNAPSE=lo:hi[:lo|uniform][:fixed][:hidden]: a learnable (or fixed) exponential synapse per neuron of
        # every hidden layer (or of every one but the first) — SNN(synapse=(lo, hi)); DESIGN.md section 6, "Synaptic
        # currents".  Every epoch logs each layer's mean and largest clamped decay.
        self.synapse = parse_synapse(os.environ.get("SPARCH_SYNAPSE"))
        if self.synapse is not None:
            if self.model_type not in ["LIF", "adLIF", "RLIF", "RadLIF"]:
                raise ValueError(f"sparch_amd: SPARCH_SYNAPSE needs a spiking model (got {self.model_type})")
            if self.tbptt is not None:
                raise ValueError("sparch_amd: SPARCH_SYNAPSE with SPARCH_TBPTT is not supported (the synaptic current "
                                 "is not carried across chunks)")
            if getattr(args, "bidirectional", False) and mode == "pack":
                raise ValueError("sparch_amd: SPARCH_SYNAPSE with --bidirectional and SPARCH_LENGTHS=pack is not "
                                 "supported")

        # SPARCH_ENCODE=code[:key=value,...]: hd / sc features are turned into spikes on the device, behind the fbank
        # (encoders.SpikeEncoder; DESIGN.md section 6, "Spike encoders"): layer 0 reads a count plane like every other
        # layer.  Every epoch logs the input spike density.
        self.encode_spec = parse_encode(os.environ.get("SPARCH_ENCODE"))
        self.encoder = None
        if self.encode_spec is not None:
            if getattr(args, "dataset_name", None) in _SPIKING_SETS:
                raise ValueError(f"sparch_amd: SPARCH_ENCODE with --dataset_name {args.dataset_name}: its input is "
                                 "already spikes (the encoders turn hd / sc features into spikes)")
            if self.model_type not in ["LIF", "adLIF", "RLIF", "RadLIF"] and not self.use_pretrained_model:
                raise ValueError(f"sparch_amd: SPARCH_ENCODE needs a spiking model (got {self.model_type})")

        self.rank, self.world, self.local_rank = dp.init_from_env()
        self.is_main = self.rank == 0
        if self.tbptt is not None and self.world > 1:  # (known only now; on every rank alike, before the first collective)
            raise ValueError("sparch_amd: SPARCH_TBPTT in a data-parallel run is not supported")
        # The HD / SC loaders (file and resident) pad each batch to its own longest clip, so ranks hold different numbers of rows
        # (B * T); the --sync_bn exchange (functional._Norm) gathers equal-sized statistics from every rank.  Refused
        # on every rank alike, before the first collective.
        if self.sync_bn and self.world > 1 and self.dataset_name in _AUDIO_SETS and not self.synthetic:
            raise ValueError("sparch_amd: --sync_bn needs the same number of time steps on every rank; the hd / sc "
                             "loaders give each batch the length of its longest clip. Run without --sync_bn "
                             "(per-rank BatchNorm statistics) or with --synthetic 1.")

        self.init_exp_folders()
        self.init_logging()
        print_model_options(args)
        print_training_options(args)

        if not torch.cuda.is_available():
            raise RuntimeError("sparch_amd: no HIP device visible; this build has no CPU training path")
        if os.environ.get("SPARCH_SHARE_GPU", "0") == "1":
            self.local_rank = 0
        self.device = torch.device("cuda", self.local_rank if self.world > 1 else 0)
        torch.cuda.set_device(self.device)
        logging.info(f"\nDevice is set to {self.device}\n")
        Fn.set_compute_dtype(self.compute_dtype)
        if self.compute_dtype != "fp32":
            logging.info("Matrix products run on bf16-rounded operands with fp32 accumulation (--compute_dtype bf16)")

        self.init_dataset()
        self.init_model()

        if self.clip_grad is None:
            self.opt = optim.Adam(self.net.parameters(), self.lr)  # exp.py:89, one launch per step (f-2)
        else:
            self.opt = optim.Adam(self.net.parameters(), self.lr, max_grad_norm=self.clip_grad)
            logging.info(f"Gradients are clipped to a global norm of {self.clip_grad} inside the optimizer step "
                         "(SPARCH_CLIP_GRAD); a step whose norm is not finite is skipped")
        self.scheduler = ReduceLROnPlateau(optimizer=self.opt, mode="max", factor=self.scheduler_factor,
                                           patience=self.scheduler_patience, min_lr=1e-6)
        self.loss_fn = Fn.CrossEntropyLoss()  # exp.py:100 (one launch for the loss and its gradient)
        self.reducer = None
        if self.world > 1:
            self.reducer = dp.GradAllReducer(self.net, rows_per_rank=self.batch_size // self.world)
            logging.info(f"Gradient all-reduce: {self.reducer.bytes_per_step / 1e6:.2f} MB per step, "
                         f"policy '{self.reducer.policy}' (sparch_amd/dp.py)")
            if self.sync_bn:
                Fn.SYNC_BN = {"group": None, "world": self.world}
                logging.info("BatchNorm statistics are exchanged between ranks (--sync_bn)")
        self.status_check_every = 64  # steps between reads of the kernels' status word (a host sync)

    # ---------------------------------------------------------------------------------- driver
    def forward(self):
        if not self.only_do_testing:
            if self.use_pretrained_model:
                logging.info("\n------ Using pretrained model ------\n")
                best_epoch, best_acc = self.valid_one_epoch(self.start_epoch, 0, 0)
            else:
                best_epoch, best_acc = 0, 0
            logging.info("\n------ Begin training ------\n")
            for e in range(best_epoch + 1, best_epoch + self.nb_epochs + 1):
                self.train_one_epoch(e)
                best_epoch, best_acc = self.valid_one_epoch(e, best_epoch, best_acc)
            logging.info(f"\nBest valid acc at epoch {best_epoch}: {best_acc}\n")
            logging.info("\n------ Training finished ------\n")
            if self.save_best:
                path = f"{self.checkpoint_dir}/best_model.pth"
                if os.path.exists(path):
                    self.net = torch.load(path, map_location=self.device, weights_only=False)  # our own file
                logging.info(f"Loading best model, epoch={best_epoch}, valid acc={best_acc}")
            else:
                logging.info("Cannot load best model because save_best option is "
                             "disabled. Model from last epoch is used for testing.")
        if self.dataset_name in ["sc", "ssc"]:
            self.test_one_epoch(self.test_loader)
        else:
            self.test_one_epoch(self.valid_loader)
            logging.info("\nThis dataset uses the same split for validation and testing.\n")

    # ---------------------------------------------------------------------------------- setup
    def init_exp_folders(self):
        if self.use_pretrained_model:
            exp_folder = self.load_exp_folder
            self.load_path = exp_folder + "/checkpoints/best_model.pth"
            if not os.path.exists(self.load_path):
                raise FileNotFoundError(errno.ENOENT, os.strerror(errno.ENOENT), self.load_path)
        elif self.new_exp_folder is not None:
            exp_folder = self.new_exp_folder
        else:
            name = "_".join([
                self.dataset_name, self.model_type,
                f"{self.nb_layers}lay{self.nb_hiddens}", f"drop{self.pdrop}", str(self.normalization),
                "bias" if self.use_bias else "nobias", "bdir" if self.bidirectional else "udir",
                "reg" if self.use_regularizers else "noreg", f"lr{self.lr}"])
            exp_folder = "exp/test_exps/" + name.replace(".", "_")
        # decided on EVERY rank (the ranks of one node see the same file system) before any collective: a
        # rank-0-only exception would leave the others waiting in the parameter broadcast
        exists = (not self.use_pretrained_model) and os.path.exists(exp_folder)
        if self.world > 1:
            flag = torch.tensor([int(exists)])
            if torch.distributed.get_backend() != "gloo":
                flag = flag.cuda()
            torch.distributed.all_reduce(flag, op=torch.distributed.ReduceOp.MAX)
            exists = bool(int(flag.item()))
        if exists:
            raise FileExistsError(errno.EEXIST, os.strerror(errno.EEXIST), exp_folder)
        if self.world > 1:  # nobody creates the folder while a peer is still looking for it
            torch.distributed.barrier()
        self.log_dir = exp_folder + "/log/"
        self.checkpoint_dir = exp_folder + "/checkpoints/"
        if self.is_main:
            os.makedirs(self.log_dir, exist_ok=True)
            os.makedirs(self.checkpoint_dir, exist_ok=True)
        self.exp_folder = exp_folder

    def init_logging(self):
        level = logging.INFO if self.is_main else logging.WARNING
        if self.log_tofile and self.is_main:
            logging.basicConfig(filename=self.log_dir + "exp.log", level=level, format="%(message)s")
        else:
            logging.basicConfig(level=level, format="%(message)s")

    def init_dataset(self):
        events_augm = ""   # SHD / SSC with --use_augm: the spec of SPARCH_EVENTS_AUGMENT (dataloaders/event_augment.py)
        if self.dataset_name in _SPIKING_SETS:
            self.nb_inputs, self.nb_outputs, kind = 700, _SPIKING_SETS[self.dataset_name], "spiking"
            events_augm = os.environ.get("SPARCH_EVENTS_AUGMENT", "") if self.use_augm else ""
            if self.use_augm and not events_augm:
                logging.warning("\nWarning: Data augmentation not implemented for SHD and SSC.\n")
            if events_augm and (self.synthetic or os.environ.get("SPARCH_EVENTS", "") != "resident"):
                raise ValueError("--use_augm with SPARCH_EVENTS_AUGMENT set augments the events inside the resident "
                                 "store's batch kernel: it needs SPARCH_EVENTS=resident and no --synthetic")
        elif self.dataset_name in _AUDIO_SETS:
            self.nb_inputs, self.nb_outputs, kind = 40, _AUDIO_SETS[self.dataset_name], "audio"
            if self.encode_spec is not None:  # the network is built for the spikes, not the 40 features
                self.encoder = SpikeEncoder.from_spec(self.encode_spec, self.nb_inputs)
                self.nb_inputs = self.encoder.out_features
                self._enc_steps = 0
        else:
            raise ValueError(f"Invalid dataset name {self.dataset_name}")
        self.input_kind = kind
        if self.batch_size % self.world != 0:
            raise ValueError(f"batch_size {self.batch_size} must be divisible by the number of GPUs {self.world}")
        per_rank = self.batch_size // self.world
        if not self.synthetic:
            # data-parallel: each rank draws its 1/world share of every epoch
            if kind == "spiking":
                from .dataloaders.spiking_datasets import load_shd_or_ssc  # exp.py:224-252 (needs h5py + the files)

                def ld(split, shuffle):
                    return load_shd_or_ssc(self.dataset_name, self.data_folder, split, per_rank, nb_steps=100,
                                           shuffle=shuffle, device=self.device, rank=self.rank, world=self.world,
                                           values=self.model_type in ("MLP", "RNN", "LiGRU", "GRU"),
                                           augment=events_augm if events_augm and split == "train" else None)
            else:
                from .dataloaders.nonspiking_datasets import load_hd_or_sc  # exp.py:254-288

                def ld(split, shuffle):
                    return load_hd_or_sc(self.dataset_name, self.data_folder, split, per_rank, shuffle=shuffle,
                                         use_augm=self.use_augm, device=self.device, rank=self.rank,
                                         world=self.world)

            self.train_loader, self.valid_loader = ld("train", True), ld("valid", False)
            if self.dataset_name in ["sc", "ssc"]:
                self.test_loader = ld("test", False)
            if self.use_augm and (kind == "audio" or events_augm):  # exp.py:285-286
                logging.info("\nData augmentation is used\n")
            return

        def mk(seed):
            return _SyntheticLoader(kind, per_rank, self.synthetic_batches, self.nb_outputs, self.seq_len,
                                    seed * 1000 + self.rank)

        self.train_loader, self.valid_loader = mk(1), mk(2)
        if self.dataset_name in ["sc", "ssc"]:
            self.test_loader = mk(3)

    def init_model(self):
        input_shape = (self.batch_size // self.world, None, self.nb_inputs)
        layer_sizes = [self.nb_hiddens] * (self.nb_layers - 1) + [self.nb_outputs]
        if self.use_pretrained_model:
            self.net = torch.load(self.load_path, map_location=self.device, weights_only=False)  # our own file
            logging.info(f"\nLoaded model at: {self.load_path}\n {self.net}\n")
            if self.encoder is not None:
                check_encode_model(self.net, self.encoder)
            if self.surrogate is not None:
                own = (f"{getattr(self.net, 'surrogate', 'boxcar')} (scale {getattr(self.net, 'surrogate_scale', None)})"
                       if getattr(self.net, "is_snn", False) else "none (not a spiking model)")
                logging.warning(f"SPARCH_SURROGATE={self.surrogate[0]} is ignored: the loaded model keeps its own "
                                f"surrogate gradient, {own}")
            if self.readout is not None:
                logging.warning(f"SPARCH_READOUT={self.readout} is ignored: the loaded model keeps its own readout")
            if self.delays is not None:
                logging.warning("SPARCH_DELAYS is ignored: the loaded model keeps its own delays (or none)")
            if self.synapse is not None:
                logging.warning("SPARCH_SYNAPSE is ignored: the loaded model keeps its own synapses (or none)")
        elif self.model_type in ["LIF", "adLIF", "RLIF", "RadLIF"]:
            name, scale = self.surrogate if self.surrogate is not None else ("boxcar", None)
            self.net = SNN(input_shape=input_shape, layer_sizes=layer_sizes, neuron_type=self.model_type,
                           dropout=self.pdrop, normalization=self.normalization, use_bias=self.use_bias,
                           bidirectional=self.bidirectional, use_readout_layer=True, surrogate=name,
                           surrogate_scale=scale, **({} if self.readout is None else {"readout": self.readout}),
                           **(self.delays or {}), **(self.synapse or {})).to(self.device)
            logging.info(f"\nCreated new spiking model:\n {self.net}\n")
            if self.synapse is not None:
                logging.info("Synaptic currents: decay in [{0:g}, {1:g}], init {syn_init}, {2}, {synapse_layers} layers "
                             "(SPARCH_SYNAPSE)".format(*self.synapse["synapse"],
                                                       "learnable" if self.synapse["learn_synapse"] else "fixed",
                                                       **self.synapse))
            if self.delays is not None:
                logging.info("Axonal delays: up to {max_delay} steps, init {delay_init}, {0}, {delay_layers} layers "
                             "(SPARCH_DELAYS)".format("learnable" if self.delays["learn_delays"] else "fixed",
                                                      **self.delays))
            if self.surrogate is not None:
                logging.info(f"Surrogate gradient: {name}" + ("" if scale is None else f", scale {scale:g}")
                             + " (SPARCH_SURROGATE)")
        elif self.model_type in ["MLP", "RNN", "LiGRU", "GRU"]:
            # exp.py:311-322: MLP and RNN on the fused / persistent kernels, LiGRU and GRU
            # launch-per-step
            self.net = ANN(input_shape=input_shape, layer_sizes=layer_sizes, ann_type=self.model_type,
                           dropout=self.pdrop, normalization=self.normalization, use_bias=self.use_bias,
                           bidirectional=self.bidirectional, use_readout_layer=True).to(self.device)
            logging.info(f"\nCreated new non-spiking model:\n {self.net}\n")
            if self.surrogate is not None:
                logging.warning(f"SPARCH_SURROGATE is ignored: {self.model_type} has no spike function")
        else:
            raise ValueError(f"Invalid model type {self.model_type}")
        if self.world > 1:  # identical initial replicas
            for p in self.net.parameters():
                torch.distributed.broadcast(p.data, src=0)
        # a resident event loader (SPARCH_EVENTS=resident) serves the bf16 plane a spiking layer 1 reads; a
        # non-spiking network reads the values themselves: dense fp32 batches there (asked for when the loaders were
        # made, from --model_type; a pretrained model says itself what it is)
        for name in ("train_loader", "valid_loader", "test_loader"):
            loader = getattr(self, name, None)
            if hasattr(loader, "store") and hasattr(loader, "values"):
                loader.values = not self.net.is_snn
        if self.encoder is not None:
            check_encode_model(self.net, self.encoder)
            logging.info(f"Input features are encoded as spikes on the device: {self.encoder} (SPARCH_ENCODE)")
        self.nb_params = sum(p.numel() for p in self.net.parameters() if p.requires_grad)
        logging.info(f"Total number of trainable parameters is {self.nb_params}")

    # ---------------------------------------------------------------------------------- epochs
    def _to_device(self, x, y, xlens=None, seed=None):
        if x.device != self.device:  # (a batch made on the device is passed on as it is, plane tag included)
            x = x.to(self.device, non_blocking=True)
        if y.device != self.device:
            y = y.to(self.device, non_blocking=True)
        if x.dtype == torch.uint8:  # spike counts as bytes: expanded on the device
            x = Fn.input_from_counts(x) if self.net.is_snn else x.float()
        if self.input_kind == "audio" and x.ndim == 2:  # synthetic waves; the file loaders deliver features
            x = fbank(x, num_mel_bins=40)  # (B, 16000) -> (B, 98, 40) on the device
        if self.encoder is not None:  # SPARCH_ENCODE: features -> the count plane layer 0 reads; padded steps emit nothing
            if xlens is not None:
                xlens = torch.as_tensor(xlens).clamp(max=x.shape[1])
                self._enc_steps = self._enc_steps + xlens.sum()
            else:
                self._enc_steps = self._enc_steps + x.shape[0] * x.shape[1]
            x = self.encoder.encode(x, lengths=xlens, seed=seed)
        return x, y

    def _log_density(self, prefix):
        """SPARCH_ENCODE: spikes per input feature and valid step since the last call (one read-back per epoch)."""
        if self.encoder is None:
            return
        spikes, steps = float(self.encoder.totals().sum()), float(self._enc_steps)
        self._enc_steps = 0
        density = self._mean_over_ranks(spikes / max(steps * self.encoder.out_features, 1.0))
        logging.info(f"{prefix} input spike density={density:.6f} spikes per feature and step "
                     f"(SPARCH_ENCODE: {self.encoder.code})")

    def _prefetched(self, loader):
        """The loader's batches, on the device, uploaded ONE BATCH AHEAD on a side stream (pinned source,
        non-blocking copy) while the compute stream runs the current step; the compute stream waits for a batch's
        event before it uses it.  In stream order (rounds 1-2) the upload sat between two steps."""
        main = torch.cuda.current_stream(self.device)
        side = getattr(self, "_upload_stream", None)
        if side is None:
            side = self._upload_stream = torch.cuda.Stream(device=self.device)

        def put(batch):
            x, xlens, y = batch
            if x.device == self.device and y.device == self.device:
                return x, xlens, y, None  # made on the device by kernels of the compute stream: nothing to upload
            with torch.cuda.stream(side):
                xd = x.to(self.device, non_blocking=True)
                yd = y.to(self.device, non_blocking=True)
                ev = torch.cuda.Event()
                ev.record(side)
            return xd, xlens, yd, ev

        it = iter(loader)
        try:
            nxt = put(next(it))
        except StopIteration:
            return
        while nxt is not None:
            xd, xlens, yd, ev = nxt
            try:
                nxt = put(next(it))
            except StopIteration:
                nxt = None
            if ev is not None:
                main.wait_event(ev)
                for t in (xd, yd):
                    if t.is_cuda:
                        t.record_stream(main)
            yield xd, xlens, yd

    def _net(self, x, xlens):
        """The network on one batch: with SPARCH_LENGTHS=mask or pack the clips' lengths go with it; with
        SPARCH_PER_STEP_LOSS the readout's running sum comes back as a third value."""
        if self.per_step_loss is not None:
            if not getattr(self.net, "is_snn", False):
                raise ValueError("sparch_amd: SPARCH_PER_STEP_LOSS needs a spiking model")
            return self.net(x, lengths=None if self.lengths_mode is None else xlens, per_step="sum")
        if self.lengths_mode is None:
            return self.net(x)
        if not getattr(self.net, "is_snn", False):
            raise ValueError("sparch_amd: SPARCH_LENGTHS needs a spiking model")
        if self.lengths_mode == "pack":
            return self.net(x, lengths=xlens, pack=True)
        return self.net(x, lengths=xlens)

    def _train_batch_tbptt(self, x, y):
        """SPARCH_TBPTT=K: one training batch as ceil(T / K) chunks of K steps.  The first chunk starts from the usual
        draw, each later one from the detached state the one before ended in; per chunk: forward, the loss on the
        chunk's own output and firing rates, backward, one optimizer step.  Returns (the mean of the chunks' losses, the
        summed output — the whole sequence's under the parameters as they moved —, the mean firing rates)."""
        from .snns import detach_state
        K, T = self.tbptt, x.shape[1]
        state, total, chunk_losses, rates = None, None, [], []
        for t0 in range(0, T, K):
            out, fr, state = self.net(Fn.time_slice(x, t0, min(t0 + K, T)), state=state, return_state=True)
            state = detach_state(state)
            loss_val = self.loss_fn(out, y)
            chunk_losses.append(loss_val.detach())
            if self.use_regularizers:
                loss_val = loss_val + self.reg_factor * (F.relu(self.reg_fmin - fr).sum() + F.relu(fr - self.reg_fmax).sum())
            self.opt.zero_grad()
            loss_val.backward()
            self.opt.step()
            self._tbptt_steps += 1
            total = out.detach() if total is None else total + out.detach()
            rates.append(fr.detach())
        return torch.stack(chunk_losses).mean(), total, torch.stack(rates).mean(dim=0)

    def _mean_over_ranks(self, value):
        if self.world == 1:
            return value
        t = torch.tensor([float(value)], device=self.device, dtype=torch.float64)
        torch.distributed.all_reduce(t)
        return float(t.item()) / self.world

    def train_one_epoch(self, e):
        start = time.time()
        self.net.train()
        if hasattr(getattr(self.train_loader, "sampler", None), "set_epoch"):
            self.train_loader.sampler.set_epoch(e)  # per-rank shards of a fresh permutation every epoch
        losses, accs, sizes = [], [], []
        early_losses = []  # SPARCH_PER_STEP_LOSS: the per-step term of every batch (unweighted)
        epoch_spike_rate = 0
        seen = 0
        # No host round trip inside the loop: the reference's per-step `.item()` / `.cpu()`
        # (exp.py:363, 381) become device-side lists read back ONCE per epoch — the same fp32 per-batch
        # values, the same float64 means — and the kernels' status word is checked at the same point.
        for step, (x, xlens, y) in enumerate(self._prefetched(self.train_loader)):
            x, y = self._to_device(x, y, xlens)  # (SPARCH_ENCODE: the encoder's own seed sequence moves on per batch)
            if self.tbptt is not None:
                loss_val, output, firing_rates = self._train_batch_tbptt(x, y)
                losses.append(loss_val)
                epoch_spike_rate += torch.mean(firing_rates)
                accs.append((y == torch.argmax(output, dim=1)).sum())
                sizes.append(y.shape[0])
                seen += x.shape[0] * x.shape[1]
                if (step + 1) % self.status_check_every == 0:
                    self._check_kernels(e, step)
                continue
            output, firing_rates, *seq = self._net(x, xlens)
            loss_val = self.loss_fn(output, y)
            losses.append(loss_val.detach())
            if seq:
                early = per_step_nll(seq[0], y, None if self.lengths_mode is None else xlens, self.per_step_loss[1])
                early_losses.append(early.detach())
                loss_val = loss_val + self.per_step_loss[0] * early
            if self.net.is_snn:
                epoch_spike_rate += torch.mean(firing_rates)
                if self.use_regularizers:
                    reg_quiet = F.relu(self.reg_fmin - firing_rates).sum()
                    reg_burst = F.relu(firing_rates - self.reg_fmax).sum()
                    loss_val = loss_val + self.reg_factor * (reg_quiet + reg_burst)
            self.opt.zero_grad()
            loss_val.backward()
            if self.reducer is not None:
                self.reducer.finish()
            self.opt.step()
            pred = torch.argmax(output, dim=1)
            accs.append((y == pred).sum())
            sizes.append(y.shape[0])
            seen += x.shape[0] * x.shape[1]
            if (step + 1) % self.status_check_every == 0:
                self._check_kernels(e, step)
        self._check_kernels(e, step)
        losses = torch.stack(losses).cpu().numpy().astype(np.float64) if losses else np.zeros(0)
        accs = (torch.stack(accs).cpu().numpy().astype(np.float64) / np.asarray(sizes, np.float64)) if accs else np.zeros(0)
        logging.info(f"Epoch {e}: lr={self.opt.param_groups[-1]['lr']}")
        logging.info(f"Epoch {e}: train loss={self._mean_over_ranks(np.mean(losses))}")
        logging.info(f"Epoch {e}: train acc={self._mean_over_ranks(np.mean(accs))}")
        if self.tbptt is not None:
            logging.info(f"Epoch {e}: SPARCH_TBPTT={self.tbptt}: optimizer steps={self._tbptt_steps}")
            self._tbptt_steps = 0  # (a per-epoch figure)
        if early_losses:
            early = torch.stack(early_losses).cpu().numpy().astype(np.float64)
            logging.info(f"Epoch {e}: train per-step loss={self._mean_over_ranks(np.mean(early))}")
        if self.clip_grad is not None:
            s = self.opt.clip_stats()
            self.opt.reset_clip_stats()  # (per-epoch figures)
            logging.info(f"Epoch {e}: grad norm max={s['max_norm']}, clipped {s['clipped']} of {s['steps']} steps, "
                         f"skipped {s['skipped']} non-finite")
        if getattr(self.net, "synapse", None) is not None:  # one read-back per epoch
            stats = torch.stack([torch.stack((g.mean(), g.max())) for g in self.net.synapse_gammas().values()]).tolist()
            for i, (mean, top) in zip(self.net.synapse_gammas(), stats):
                logging.info(f"Epoch {e}: layer {i} synapse: mean gamma={mean:.4f}, max gamma={top:.4f}")
        if getattr(self.net, "max_delay", 0):  # one read-back per epoch; the forward never reads the delays on the host
            for i, d in self.net.delay_steps().items():
                logging.info(f"Epoch {e}: layer {i} delays: mean d={float(d.float().mean()):.3f}, max d={int(d.max())} "
                             f"(of {self.net.max_delay})")
        self._log_density(f"Epoch {e}: train")
        if self.net.is_snn:
            epoch_spike_rate /= step  # sic: the reference divides by the last batch index (exp.py:398)
            logging.info(f"Epoch {e}: train mean act rate={epoch_spike_rate}")
        elapsed = time.time() - start
        logging.info(f"Epoch {e}: train elapsed time={str(timedelta(seconds=elapsed))}")
        logging.info(f"Epoch {e}: train throughput={self.world * seen / elapsed:.0f} timesteps*samples/s")

    def _check_kernels(self, e, step):
        """Read the recurrent kernels' status word.  After an in-kernel timeout (the persistent grid could
        not become co-resident: GPU shared or partitioned) the steps since the last check were no-ops on the
        device (the optimizer and the BatchNorm statistics skip themselves while the word is raised); this
        process now continues with one launch per time step — new launches, same process.  With SPARCH_CLIP_GRAD the
        same read takes back the steps skipped for a non-finite gradient norm (every rank skipped the same ones)."""
        if self.clip_grad is not None:
            n = self.opt.sync_skipped()
            if n:
                logging.warning(f"Epoch {e}, step {step}: {n} step(s) had a NaN or inf gradient norm and were skipped")
        if self._timeout_on_any_rank():
            logging.warning(f"Epoch {e}, step {step}: {Fn._TIMEOUT_TEXT}  [{Fn.describe_timeout()}]  Steps since the "
                            "timeout were skipped on every rank; continuing with one kernel launch per time step "
                            "(SPARCH_REC_STEPS_PER_LAUNCH=1 behaviour).")

    def _timeout_on_any_rank(self):
        """Collective read of the status word: every rank sees the MAX over ranks (the reducer already merges it
        every training step; evaluation has no reducer), so all ranks degrade together — a rank that raised
        alone used to leave its peers waiting in the next collective.  After a degrade the replicas are
        re-synchronised from rank 0 (they skipped the same steps, so this is a safety net, not a repair)."""
        if self.world > 1:
            dp.sync_status(self.device)
        if not check_status(self.device, on_timeout="degrade"):
            return False
        if self.world > 1:
            for t in list(self.net.parameters()) + list(self.net.buffers()):
                torch.distributed.broadcast(t.data, src=0)
        return True

    def _eval_epoch(self, loader, retried=False):
        losses, accs, sizes = [], [], []
        decided = []  # SPARCH_PER_STEP_LOSS: the sum of the clips' decision steps, per batch
        self.decision_step = None
        epoch_spike_rate = 0
        step = 0
        # SPARCH_ENCODE: an evaluation repeats — the seed of a batch comes from the split and the batch's index
        split = 1 if loader is self.valid_loader else 2
        for step, (x, xlens, y) in enumerate(self._prefetched(loader)):
            seed = None if self.encoder is None else _mix64(_mix64(self.encoder.base_seed, -1 - split), step)
            x, y = self._to_device(x, y, xlens, seed)
            output, firing_rates, *seq = self._net(x, xlens)
            losses.append(self.loss_fn(output, y).detach())
            if seq:
                decided.append(decision_steps(seq[0], y, None if self.lengths_mode is None else xlens).sum())
            pred = torch.argmax(output, dim=1)
            accs.append((y == pred).sum())
            sizes.append(y.shape[0])
            if self.net.is_snn:
                epoch_spike_rate += torch.mean(firing_rates)
        if self._timeout_on_any_rank():  # the epoch's numbers are invalid: once more, now with per-step launches
            if retried:
                raise Fn._capi.SparchHipError(Fn._TIMEOUT_TEXT + "  [" + Fn.describe_timeout() + "]")
            logging.warning(f"Evaluation: {Fn._TIMEOUT_TEXT}  [{Fn.describe_timeout()}]  Repeating the epoch with one "
                            "kernel launch per time step.")
            return self._eval_epoch(loader, retried=True)
        losses = torch.stack(losses).cpu().numpy().astype(np.float64) if losses else np.zeros(0)
        accs = (torch.stack(accs).cpu().numpy().astype(np.float64) / np.asarray(sizes, np.float64)) if accs else np.zeros(0)
        if decided:  # the mean over the clips of the epoch
            self.decision_step = self._mean_over_ranks(float(torch.stack(decided).sum().item()) / max(sum(sizes), 1))
        if self.net.is_snn:
            epoch_spike_rate /= step  # sic (exp.py:449, 515)
        return (self._mean_over_ranks(np.mean(losses)), self._mean_over_ranks(np.mean(accs)), epoch_spike_rate)

    def valid_one_epoch(self, e, best_epoch, best_acc):
        with torch.no_grad():
            self.net.eval()
            valid_loss, valid_acc, rate = self._eval_epoch(self.valid_loader)
            logging.info(f"Epoch {e}: valid loss={valid_loss}")
            logging.info(f"Epoch {e}: valid acc={valid_acc}")
            if self.decision_step is not None:
                logging.info(f"Epoch {e}: valid mean decision step={self.decision_step}")
            self._log_density(f"Epoch {e}: valid")
            if self.net.is_snn:
                logging.info(f"Epoch {e}: valid mean act rate={rate}")
            self.scheduler.step(valid_acc)
            if valid_acc > best_acc:
                best_acc, best_epoch = valid_acc, e
                if self.save_best and self.is_main:
                    torch.save(self.net, f"{self.checkpoint_dir}/best_model.pth")
                    logging.info(f"\nBest model saved with valid acc={valid_acc}")
            if self.world > 1:
                torch.distributed.barrier()
            logging.info("\n-----------------------------\n")
            return best_epoch, best_acc

    def test_one_epoch(self, test_loader):
        with torch.no_grad():
            self.net.eval()
            logging.info("\n------ Begin Testing ------\n")
            test_loss, test_acc, rate = self._eval_epoch(test_loader)
            logging.info(f"Test loss={test_loss}")
            logging.info(f"Test acc={test_acc}")
            if self.decision_step is not None:
                logging.info(f"Test mean decision step={self.decision_step}")
            self._log_density("Test")
            if self.net.is_snn:
                logging.info(f"Test mean act rate={rate}")
            logging.info("\n-----------------------------\n")
