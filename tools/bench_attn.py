"""Key-tiled attention kernels at the bench shape (32 x 376 frames, 4 heads of 64): forward with / without dropout, backward.
--window W [W ...]: forward and backward of full attention against local attention [W, W] (the kernels of csrc/attention_flash.hip and
attention_flash_bwd.hip under their local span) at --shape (default 1 x T x 8 heads of 64 for T = 751, 3001, 15001: 30 s, 2 min and 10 min of audio),
outputs and scratch preallocated and the C entry points called directly so that the window times launches, not allocations.
The full backward is skipped at a shape only if its dBand does not fit in free device memory.  Developer tool."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timeit(fn, n=50):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n * 1e3


def _operands(B, T, H, dk, rows, g):
    d = H * dk
    qkv = (torch.randn(B * T, 3 * d, generator=g) * 0.8).bfloat16().cuda()
    pl = (torch.randn(rows, d, generator=g) * 0.8).bfloat16().cuda()
    bu = (torch.randn(H, dk, generator=g) * 0.3).cuda(); bv = (torch.randn(H, dk, generator=g) * 0.3).cuda()
    return qkv, pl, bu, bv


def bench_window(shapes, windows, n):
    """Full against local forward.  The full kernel's table is built here for the T at hand (2T-1 rows): nothing depends on a
    model's pos_emb_max_len.  The local table is the centre 2w+1 rows of the same one, so a window >= T-1 computes the same."""
    from indic_cl_asr_amd import _lib
    L, P = _lib.lib(), _lib.ptr
    for B, T, H, dk in shapes:
        g = torch.Generator().manual_seed(0)
        qkv, pl, bu, bv = _operands(B, T, H, dk, 2 * T - 1, g)
        lens = torch.full((B,), T, dtype=torch.int64).cuda()
        ctx = torch.empty(B * T, H * dk, dtype=torch.bfloat16, device="cuda")
        st = _lib.stream_ptr()

        def full():
            _lib.check(L.ia_relpos_attention_flash(P(qkv), P(pl), P(bu), P(bv), P(lens), B, T, H, dk, 0.0, 0, P(ctx), st), "full")

        t_full = timeit(full, n)
        nqt = (T + 63) // 64
        print(f"B {B} T {T} H {H} dk {dk}: full {t_full:9.1f} us  ({B * H * nqt} workgroups x {nqt} key tiles)", flush=True)
        for w in windows:
            wc = min(w, T - 1)
            plw = pl[T - 1 - wc: T + wc].contiguous()

            def local():
                _lib.check(L.ia_relpos_attention_local(P(qkv), P(plw), P(bu), P(bv), P(lens), B, T, H, dk, wc, 0.0, 0, P(ctx), st),
                           "local")

            t_loc = timeit(local, n)
            print(f"    local [{w},{w}] {t_loc:9.1f} us   full / local = {t_full / t_loc:5.2f}   "
                  f"(<= {1 + 2 * ((wc + 63) // 64)} key tiles per workgroup)", flush=True)
        bench_window_bwd(B, T, H, dk, qkv, pl, bu, bv, lens, windows, n)


def bench_window_bwd(B, T, H, dk, qkv, pl, bu, bv, lens, windows, n):
    """Full against local backward (all launches of one C call: memset, query-owner, key-owner, bias finish, TN GEMM, pack)."""
    import ctypes
    from indic_cl_asr_amd import _lib
    from indic_cl_asr_amd.ops import fast
    L, P = _lib.lib(), _lib.ptr
    d = H * dk
    st = _lib.stream_ptr()
    bf = dict(dtype=torch.bfloat16, device="cuda")
    dctx = (torch.randn(B * T, d, generator=torch.Generator().manual_seed(1)) * 0.5).bfloat16().cuda()
    dqkv, QvHM = torch.empty(B * T, 3 * d, **bf), torch.empty(H * B * T * 64, **bf)
    dub = torch.empty(2, H, dk, device="cuda")
    n = max(10, n // 4)
    Rs, _ = fast.attention_flash_bwd_dims(T)
    need = H * B * T * Rs * 2
    free = torch.cuda.mem_get_info()[0]
    t_full = None
    if need > 0.9 * free:
        print(f"    full backward skipped: its dBand [H, B*T, {Rs}] needs {need / 2**30:.1f} GiB, {free / 2**30:.1f} GiB free", flush=True)
    else:
        ctx, lse = fast.relpos_attention_flash(qkv, pl, bu, bv, lens, B, T, H, dk, want_lse=True)
        dBand, dpl = torch.empty(H * B * T * Rs, **bf), torch.empty_like(pl)
        ws = torch.empty(L.ia_relpos_attention_flash_bwd_ws_elems(B, T, H, dk), device="cuda")

        def full():
            _lib.check(L.ia_relpos_attention_flash_bwd(P(qkv), P(pl), P(bu), P(bv), P(lens), P(ctx), P(dctx), P(lse), B, T, H, dk, 0.0, 0,
                                                       P(dqkv), P(dpl), pl.shape[0], P(dub[0]), P(dub[1]), P(dBand), P(QvHM), P(ws), st),
                       "full bwd")

        t_full = timeit(full, n)
        print(f"    full backward  {t_full:9.1f} us   (dBand row {Rs}: {need / 2**20:.0f} MiB)", flush=True)
        del dBand, ws
    for w in windows:
        wc = min(w, T - 1)
        plw = pl[T - 1 - wc: T + wc].contiguous()
        ctx, lse = fast.relpos_attention_local(qkv, plw, bu, bv, lens, B, T, H, dk, wc, want_lse=True)
        Rl, _ = fast.attention_local_bwd_dims(T, wc)
        dBand, dpl = torch.empty(H * B * T * Rl, **bf), torch.empty_like(plw)
        ws = torch.empty(L.ia_relpos_attention_local_bwd_ws_elems(B, T, H, dk, wc), device="cuda")

        def local():
            _lib.check(L.ia_relpos_attention_local_bwd(P(qkv), P(plw), P(bu), P(bv), P(lens), P(ctx), P(dctx), P(lse), B, T, H, dk, wc,
                                                       0.0, 0, P(dqkv), P(dpl), plw.shape[0], P(dub[0]), P(dub[1]), P(dBand), P(QvHM),
                                                       P(ws), st), "local bwd")

        t_loc = timeit(local, n)
        ratio = f"full / local = {t_full / t_loc:6.2f}" if t_full else "(no full backward)"
        print(f"    local backward [{w},{w}] {t_loc:9.1f} us   {ratio}   (dBand row {Rl}: {H * B * T * Rl * 2 / 2**20:.1f} MiB)", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=int, nargs="+", default=None, help="time full against local attention [W, W] (forward)")
    ap.add_argument("--shape", type=int, nargs=4, action="append", metavar=("B", "T", "H", "DK"), default=None)
    ap.add_argument("--iters", type=int, default=200)
    args = ap.parse_args()
    if args.window:
        bench_window(args.shape or [(1, 751, 8, 64), (1, 3001, 8, 64), (1, 15001, 8, 64)], args.window, args.iters)
        return
    from indic_cl_asr_amd.ops import fast
    B, T, H, dk = 32, 376, 4, 64
    d = H * dk
    g = torch.Generator().manual_seed(0)
    qkv, pl, bu, bv = _operands(B, T, H, dk, 2 * T - 1, g)
    lens = torch.round(T * (0.6 + 0.4 * torch.rand(B, generator=g))).long(); lens[0] = T
    lens = lens.cuda()
    dctx = torch.randn(B * T, d, device="cuda").bfloat16()
    for p in (0.0, 0.1):
        t_f = timeit(lambda: fast.relpos_attention_flash(qkv, pl, bu, bv, lens, B, T, H, dk, dropout_p=p, seed=3))
        ctx, lse = fast.relpos_attention_flash(qkv, pl, bu, bv, lens, B, T, H, dk, dropout_p=p, seed=3, want_lse=True)
        t_b = timeit(lambda: fast.relpos_attention_flash_bwd(qkv, pl, bu, bv, lens, ctx, dctx, lse, B, T, H, dk, dropout_p=p, seed=3))
        print(f"dropout {p}: forward {t_f:6.1f} us   backward (all launches) {t_b:6.1f} us", flush=True)


if __name__ == "__main__":
    main()
