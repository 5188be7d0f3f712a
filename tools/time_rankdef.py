"""Developer tool (GPU): the GSL form of the rank-deficient covariance, device route (lsqamd_op_pivoted_inverse_dev ->
csrc/rankdef_dev.hip) against the host arithmetic (lsqamd_op_truncated_inverse -> csrc/rankdef.hip pivoted_inverse, one core).
Inputs: G = J^T J of a seeded normal J (2 P x P, column scales over 1e3) with `dropped` columns that are 0.5 x another.

Per (P, dropped): device time from HIP events (one warm-up, then the median of `repeats` calls, the copy of G into the
work matrix included), the host's wall time (one call; none above `host_max`), their ratio, the rank the device found, and
from one further traced call the device time of the pivot-chain launches (pstrf_panel_kernel), the trailing updates
(pstrf_trail_kernel) and everything else (gather, potrf_upper, trtri, gemm, symmetrise, scatter).

    python tools/time_rankdef.py [repeats] [host_max] [P ...]      e.g.  3 2048 128 512 1024 2048 4096
"""
import ctypes as C
import sys
import time

import numpy as np
import torch

sys.path.insert(0, '.')
from lsqfit_amd import _lib

repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 3
host_max = int(sys.argv[2]) if len(sys.argv) > 2 else 2048
sizes = [int(v) for v in sys.argv[3:]] or [128, 512, 1024, 2048, 4096]
lib = _lib.load()
ptr = lambda t: C.c_void_p(t.data_ptr())

for P in sizes:
    for dropped in (1, P // 2):
        rng = np.random.default_rng(P + dropped)
        J = rng.standard_normal((2 * P, P)) * 10.0 ** rng.uniform(-1.5, 1.5, P)
        J[:, P - dropped:] = 0.5 * J[:, :dropped]
        G = J.T @ J
        dG0 = torch.from_numpy(G).cuda()
        dG, cov = torch.empty_like(dG0), torch.empty_like(dG0)
        perm = torch.empty(P, dtype=torch.int32, device='cuda')
        rank = torch.empty(2, dtype=torch.int32, device='cuda')
        wb = lib.lsqamd_op_pivoted_inverse_dev_work_bytes(P)
        work = torch.empty(wb // 8 + 1, dtype=torch.float64, device='cuda')

        def call():
            dG.copy_(dG0)
            st = torch.cuda.current_stream().cuda_stream
            rc = lib.lsqamd_op_pivoted_inverse_dev(C.c_void_p(st), ptr(dG), P, P, ptr(cov), P, ptr(perm), ptr(rank), ptr(work), wb)
            assert rc == 0, rc

        ms = []
        for it in range(repeats + 1):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            call()
            b.record()
            torch.cuda.synchronize()
            if it:
                ms.append(a.elapsed_time(b))
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            call()
            torch.cuda.synchronize()
        t = dict(panel=0.0, trail=0.0, other=0.0)
        for e in prof.key_averages():
            us = getattr(e, 'device_time_total', None) or getattr(e, 'cuda_time_total', 0.0)
            t['panel' if 'pstrf_panel_kernel' in e.key else 'trail' if 'pstrf_trail_kernel' in e.key else 'other'] += us
        host, same = float('nan'), '-'
        if P <= host_max:
            out, k = np.empty((P, P)), C.c_int32(-1)
            t0 = time.perf_counter()
            assert lib.lsqamd_op_truncated_inverse(_lib.dptr(G), P, 2 * P, 0, _lib.dptr(out), C.byref(k)) == 0
            host = 1e3 * (time.perf_counter() - t0)
            same = 'yes' if np.array_equal(out.any(axis=1), cov.cpu().numpy().any(axis=1)) else 'NO'
        d = float(np.median(ms))
        print('P %4d  dropped %4d  rank %4d  status %d   device %9.2f ms [%9.2f, %9.2f]   host %11.2f ms   host / device %8.2f   same kept set %s'
              '   pivot chain %9.2f ms   trailing updates %8.2f ms   other kernels %7.2f ms'
              % (P, dropped, int(rank[0]), int(rank[1]), d, min(ms), max(ms), host, host / d, same, 1e-3 * t['panel'], 1e-3 * t['trail'],
                 1e-3 * t['other']), flush=True)
