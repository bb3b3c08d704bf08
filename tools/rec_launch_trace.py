#!/usr/bin/env python3
"""Launch geometry of the recurrent entry points, for comparing two builds of the library.

Run once per library under a kernel trace (no counters in the same run), the library chosen with SPARCH_HIP_LIB:
    rocprofv3 --kernel-trace --output-format csv -d OUT -- python3 tools/rec_launch_trace.py > OUT.calls.txt
    python3 tools/rec_launch_trace.py --summarize OUT > OUT.trace.txt
The first prints one line per call with its return code; the second the ordered sequence of (kernel, grid, workgroup)
from the trace, fill kernels included, run-length compressed, and a SHA-256 over the uncompressed sequence.  Two builds
that cut every pass into the same launches of the same kernels give identical files.  The numbers the kernels compute
are not looked at (every input is zero): what a shape launches is, e.g. one launch or two, 32- or 64-column kernels.

Every persistent entry point at T = 5: hidden sizes 32, 256, 512, 1024 (the four kgw classes) and 96 (an odd number of
column tiles), 32 rows and just over one launch group for the device's CU count, steps_per_launch 5, 2 and 1; spiking
kinds in both operand precisions with fp32 and bf16 saves, the stream forward, 512 rows at H = 1024 in bf16 mode (the
64-column launch); the dense cell with its three activations; LiGRU and GRU; and the step entries."""
import csv
import glob
import hashlib
import itertools
import sys

T = 5
HS = (32, 96, 256, 512, 1024)


def summarize(d):
    f = sorted(glob.glob(f"{d}/**/*kernel_trace.csv", recursive=True))[0]
    rows = sorted(csv.DictReader(open(f)), key=lambda r: (int(r["Start_Timestamp"]), int(r.get("Dispatch_Id", 0))))

    def dims(r, what):
        return "x".join(r[k] for k in sorted(r) if k.startswith(what))
    seq = [f'{r["Kernel_Name"]}  grid {dims(r, "Grid_Size")}  wg {dims(r, "Workgroup_Size")}' for r in rows]
    print(f"{len(seq)} kernels, sha256 of the sequence {hashlib.sha256(chr(10).join(seq).encode()).hexdigest()}")
    for line, run in itertools.groupby(seq):
        n = len(list(run))
        print(line if n == 1 else f"{line}  (x{n})")


def main():
    import torch

    from sparch_amd._capi import lib

    dev = torch.device("cuda", 0)
    cus = lib.sparch_device_cus()
    pool = [torch.zeros(8 << 20, dtype=torch.float32, device=dev) for _ in range(20)]     # every operand: zeros, ample
    status = torch.zeros(4, dtype=torch.int32, device=dev)
    P = [t.data_ptr() for t in pool]
    ST = status.data_ptr()

    def buf(nbytes):
        return torch.zeros(max(nbytes, 16) // 4 + 4, dtype=torch.float32, device=dev)

    def say(what, rc):
        print(f"{what} -> {rc}", flush=True)

    def over(H, per_tile, extra):          # just over one launch group: a second group with a short last row tile
        return 32 * max(cus // per_tile, 1) + extra

    # ---- spiking kinds
    for kind, prec, H in itertools.product((2, 3), (0, 1), HS):
        shapes = [32, over(H, -(-H // 32), 4)] + ([512] if (H, prec) == (1024, 1) else [])
        vf, vb = buf(lib.sparch_vpack_bytes(H)), buf(lib.sparch_vpack_bytes(H))
        say(f"vpack_both H={H} prec={prec}", lib.sparch_vpack_both(H, P[0], vf.data_ptr(), vb.data_ptr(), None, None, prec))
        for Bp, L in itertools.product(shapes, (T, 2, 1)):
            nb = lib.sparch_rec_chan_bytes(Bp, T, H)
            chan = buf(nb)
            tag = f"kind={kind} prec={prec} H={H} Bp={Bp} L={L}"
            for s16 in (0, 1):
                say(f"rec_cell_fwd {tag} save_bf16={s16}", lib.sparch_rec_cell_fwd(
                    kind, Bp, 1, T, H, P[0], None, None, P[1], P[2], P[3], P[4], vf.data_ptr(), P[5], P[6], P[7], P[8],
                    1.0, 0.0, 1, P[9], None, P[10], P[11], s16, None, chan.data_ptr(), nb, ST, L, None, prec))
                say(f"rec_cell_bwd {tag} save_bf16={s16}", lib.sparch_rec_cell_bwd(
                    kind, Bp, 1, T, H, P[0], None, P[10], P[11], s16, P[1], P[2], P[3], P[4], vb.data_ptr(), P[6], P[7],
                    P[8], 1.0, 0.0, 1, P[12], P[13], P[14], None, None, None, chan.data_ptr(), nb, ST, L, None, prec))
            say(f"rec_cell_stream_fwd {tag}", lib.sparch_rec_cell_stream_fwd(
                kind, Bp, 1, T, H, P[0], None, None, P[1], P[2], P[3], P[4], vf.data_ptr(), P[5], P[6], P[7], P[8], P[15],
                1.0, 0.0, P[9], None, None, chan.data_ptr(), nb, ST, L, None, prec))
        Bp = shapes[1]
        for t in (0, T - 1):
            say(f"rec_cell_step_fwd kind={kind} H={H} Bp={Bp} t={t}", lib.sparch_rec_cell_step_fwd(
                kind, Bp, 1, T, H, t, P[0], None, None, P[1], P[2], P[3], P[4], P[5], P[6], P[7], P[8], 1.0, 0.0, 1, P[9],
                None, P[10], P[11], None, P[15], None))
            say(f"rec_cell_step_stream_fwd kind={kind} H={H} Bp={Bp} t={t}", lib.sparch_rec_cell_step_stream_fwd(
                kind, Bp, 1, T, H, t, P[0], None, None, P[1], P[2], P[3], P[4], P[5], P[6], P[7], P[8], P[15], 1.0, 0.0,
                P[9], None, None, None))
            say(f"rec_cell_step_bwd kind={kind} H={H} Bp={Bp} t={t}", lib.sparch_rec_cell_step_bwd(
                kind, Bp, 1, T, H, t, P[0], None, P[10], P[11], P[1], P[2], P[3], P[4], P[5], P[6], P[7], P[8], 1.0, 0.0,
                1, P[12], P[13], P[14], None, None, None, P[16], None))

    # ---- dense cell
    for act, H in itertools.product((0, 1, 2), HS):
        vp = buf(lib.sparch_vpack_bytes(H))
        say(f"vpack H={H}", lib.sparch_vpack(H, P[0], 1 | 2, vp.data_ptr(), None, None, 0))
        for Bp, L in itertools.product((32, over(H, -(-H // 32), 4)), (T, 2, 1)):
            nb = lib.sparch_rec_chan_bytes(Bp, T, H)
            chan = buf(nb)
            tag = f"act={act} H={H} Bp={Bp} L={L}"
            say(f"ann_rec_fwd {tag}", lib.sparch_ann_rec_fwd(act, Bp, 1, T, H, P[0], None, None, vp.data_ptr(), 0.0, 1, P[1],
                                                            P[2], chan.data_ptr(), nb, ST, L, None))
            say(f"ann_rec_bwd {tag}", lib.sparch_ann_rec_bwd(act, Bp, 1, T, H, P[0], P[2], vp.data_ptr(), 0.0, 1, P[3], P[4],
                                                            chan.data_ptr(), nb, ST, L, None))
        Bp = over(H, -(-H // 32), 4)
        for s in (0, T - 1):
            say(f"ann_rec_step_fwd act={act} H={H} Bp={Bp} s={s}", lib.sparch_ann_rec_step_fwd(
                act, Bp, 1, T, H, s, P[0], None, None, P[5], 0.0, 1, P[1], P[2], P[6], None))
            say(f"ann_rec_step_bwd act={act} H={H} Bp={Bp} s={s}", lib.sparch_ann_rec_step_bwd(
                act, Bp, 1, T, H, s, P[0], P[2], P[5], 0.0, 1, P[3], P[4], P[6], None))

    # ---- gated cells
    for H in HS:
        vl = [buf(lib.sparch_ligru_vpack_bytes(H, b)) for b in (0, 1)]
        vg = [[buf(lib.sparch_gru_vpack_bytes(H, b, w)) for w in (0, 1)] for b in (0, 1)]
        for b in (0, 1):
            say(f"ligru_vpack H={H} bwd={b}", lib.sparch_ligru_vpack(H, P[0], P[1], b, vl[b].data_ptr(), None, 0))
            say(f"gru_vpack H={H} bwd={b}", lib.sparch_gru_vpack(H, P[0], P[1], P[2], b, vg[b][0].data_ptr(),
                                                                  vg[b][1].data_ptr(), None, 0))
        for Bp, L in itertools.product((32, over(H, H // 16, 2)), (T, 2, 1)):
            tag = f"H={H} Bp={Bp} L={L}"
            nb = lib.sparch_ligru_chan_bytes(Bp, H)
            chan = buf(nb)
            say(f"ligru_fwd {tag}", lib.sparch_ligru_fwd(Bp, 1, T, H, P[0], None, None, P[1], None, None, vl[0].data_ptr(), 0.0,
                                                        1, P[2], P[3], P[4], P[5], chan.data_ptr(), nb, ST, L, None))
            say(f"ligru_bwd {tag}", lib.sparch_ligru_bwd(Bp, 1, T, H, P[0], P[3], P[4], P[5], vl[1].data_ptr(), 0.0, 1, P[6],
                                                        P[7], P[8], P[9], chan.data_ptr(), nb, ST, L, None))
            nb = lib.sparch_gru_chan_bytes(Bp, H)
            chan = buf(nb)
            say(f"gru_fwd {tag}", lib.sparch_gru_fwd(Bp, 1, T, H, P[0], None, None, P[1], None, None, P[10], None, None,
                                                    vg[0][0].data_ptr(), vg[0][1].data_ptr(), 0.0, 1, P[2], P[3], P[4],
                                                    P[11], P[5], chan.data_ptr(), nb, ST, L, None))
            say(f"gru_bwd {tag}", lib.sparch_gru_bwd(Bp, 1, T, H, P[0], P[3], P[4], P[11], P[5], vg[1][0].data_ptr(),
                                                    vg[1][1].data_ptr(), 0.0, 1, P[6], P[12], P[7], P[8], P[13], P[9],
                                                    chan.data_ptr(), nb, ST, L, None))
    torch.cuda.synchronize()
    print(f"cus {cus}  status word {status.tolist()}")


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--summarize":
        summarize(sys.argv[2])
    else:
        main()
