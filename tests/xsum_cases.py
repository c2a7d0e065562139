"""What the tests of rot_shift2D + class sums (csrc/ralign_xform.h) share: the run count of the launch plan and the poses at
the arithmetic's edges."""


def xs_runs(n, nseg, nx=0):
    """runs every (class, parity) list of a batch of n particles is cut into by transform_sum_db_kernel / transform_sum_kernel /
    transform_sum_tile_kernel: xs_runs(xs_plan(nx), nseg, n) in csrc/ralign_engine.hip, restated"""
    nrun = max(1, min(512, (1024 + nseg - 1) // nseg))
    if nx > 141:          # output tiles of 64 x 64 pixels: that many workgroups per run already
        nrun = max(1, min(64, 2048 // (nseg * ((nx + 63) // 64) ** 2)))
    return max(1, min(nrun, n // (8 * nseg)))


def edge_poses(nx):
    """(alpha, sx, sy): angles at multiples of 90 degrees, shifts beyond +-nx (the wrap loops of xf_pose), sources outside the
    image (the background rule)"""
    return [(0.0, 0.0, 0.0), (90.0, 0.5, -0.5), (180.0, 1.0, 2.0), (270.0, -1.5, 0.25), (360.0, 0.0, 0.0), (-90.0, 2.0, -2.0),
            (12.5, nx + 1.25, 0.5), (200.0, -0.75, -(2 * nx + 0.5)), (45.0, float(nx), -float(nx)), (33.0, -(nx + 2.0), 3 * nx + 0.125),
            (45.0, nx / 2 - 1.0, nx / 2 - 1.0), (135.0, -(nx / 2 - 1.5), 0.0), (0.0, 0.5, 0.5), (90.0, nx - 0.5, 0.0)]
