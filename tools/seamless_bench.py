"""Timing of the seamless canvas composite: profiles/seamless_bench.json.  Reports only; nothing is asserted on a time.

Two windows on a 1024 x 2048 photo canvas: composite_bench's 401 x 397 joint-edit window at an unaligned origin, and a
1021 x 2045 window (interior 1019 x 2043, all four sides counted).  Between two HIP events, the median of ``--reps`` calls
after 5 warm-up calls, all in one process:

  basis_ms   him_membrane_basis for both axes of the window (uncached: what the first paste of a shape pays once)
  solve_ms   him_membrane_solve on resident bases and workspace (five launches, the two GEMMs among them)
  fp64_tflops_over_solve   3 channels x 2 ny nx (ny + nx) flops of the two GEMM passes over solve_ms: the whole call's
             time, so a LOWER bound of the GEMM kernel's own rate
  apply_alpha1_ms / apply_border_ms   him_canvas_seamless_apply with feather 0 and with the border matte (feather 8)
  paste_ms   the whole ops.canvas_paste_seamless call (table upload, both bicubic passes, solve, apply)

Clocks are left as found and nothing is set on the device.

    python tools/seamless_bench.py [--reps 20] [--out profiles/seamless_bench.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
HC, WC, PATCH = 1024, 2048, 256
WINDOWS = {'joint_edit_401x397': (813, 307, 401, 397), 'near_canvas_1021x2045': (2, 1, 1021, 2045)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'seamless_bench.json'))
    args = ap.parse_args()
    import numpy as np
    import torch
    from composite_bench import timed
    from neurips18_hierchical_image_manipulation_amd import ops
    from neurips18_hierchical_image_manipulation_amd._cabi import lib
    assert torch.cuda.is_available(), 'seamless_bench needs the GPU'
    g = np.random.default_rng(0)
    photo = torch.from_numpy(g.random((1, 3, HC, WC), dtype=np.float32)).cuda()
    patch = torch.from_numpy(g.random((1, 3, PATCH, PATCH), dtype=np.float32)).cuda()
    box = (0, 0, PATCH, PATCH)
    st = torch.cuda.current_stream().cuda_stream
    windows = {}
    for name, (x0, y0, H, W) in WINDOWS.items():
        l, r, t, b, ny, nx = ops.membrane_sides(HC, WC, x0, y0, H, W)
        P = torch.empty((1, 3, H, W), dtype=torch.float32, device=photo.device)
        ops.canvas_paste_bicubic(patch, box, P, 0, 0, H, W)
        (Vy, Vyt, lamy), (Vx, Vxt, lamx) = ops.membrane_basis(ny, t, b), ops.membrane_basis(nx, l, r)
        scratch = [torch.empty_like(v) for v in (Vy, Vyt, lamy, Vx, Vxt, lamx)]
        m, status = ops.membrane_solve(photo, x0, y0, P)
        ws = ops._SCRATCH['membrane_solve', torch.cuda.current_device()].buf
        work = photo.clone()
        matte = torch.empty((H, W), dtype=torch.float32, device=photo.device)

        def basis():
            lib.him_membrane_basis(ny, t, b, scratch[0].data_ptr(), scratch[1].data_ptr(), scratch[2].data_ptr(), st)
            lib.him_membrane_basis(nx, l, r, scratch[3].data_ptr(), scratch[4].data_ptr(), scratch[5].data_ptr(), st)

        def solve():
            lib.him_membrane_solve(photo.data_ptr(), HC, WC, x0, y0, H, W, P.data_ptr(), Vy.data_ptr(), Vyt.data_ptr(),
                                   lamy.data_ptr(), Vx.data_ptr(), Vxt.data_ptr(), lamx.data_ptr(), m.data_ptr(),
                                   ws.data_ptr(), status.data_ptr(), st)

        def apply(feather):
            lib.him_canvas_seamless_apply(P.data_ptr(), m.data_ptr(), work.data_ptr(), HC, WC, x0, y0, H, W, 0, feather, 0, 1,
                                          matte.data_ptr(), st)

        # results first: the kernel-level calls equal the ops path, and two solves give the same bits
        keep = m.clone()
        solve()
        assert torch.equal(m, keep)
        apply(0)
        want, _, _ = ops.canvas_paste_seamless(patch, box, photo.clone(), x0, y0, H, W, 0)
        assert torch.equal(work, want)
        times = {'basis_ms': timed(basis, args.reps), 'solve_ms': timed(solve, args.reps),
                 'apply_alpha1_ms': timed(lambda: apply(0), args.reps), 'apply_border_ms': timed(lambda: apply(8), args.reps),
                 'paste_ms': timed(lambda: ops.canvas_paste_seamless(patch, box, work, x0, y0, H, W, 0), args.reps)}
        flops = 3 * 2.0 * ny * nx * (ny + nx)
        windows[name] = {'origin': [x0, y0], 'window': [H, W], 'interior': [ny, nx], 'times': times, 'gemm_flops': flops,
                         'fp64_tflops_over_solve': round(flops / (times['solve_ms']['median'] * 1e-3) / 1e12, 3)}
    out = {'device': torch.cuda.get_device_name(0), 'reps': args.reps, 'warmup': 5, 'canvas': [HC, WC], 'patch': PATCH,
           'windows': windows,
           'note': ('event-timed medians of single calls after 5 warm-up calls, one process; fp64_tflops_over_solve divides '
                    'the flops of the two GEMM passes by the time of the WHOLE solve call (ring, matvecs, scaling included), '
                    'so it is a lower bound of the GEMM kernel\'s own rate; the GEMM kernel was not timed alone and no '
                    'hardware counters were collected')}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write('\n')
    print(json.dumps(out))


if __name__ == '__main__':
    main()
