#!/usr/bin/env python3
"""List-scheduling model of a launch over the sorted ray slots of limb_1e6: what the order in which the workgroups are
handed out costs (the block order).  CPU only; prints one table.

The rays are drawn like the bench's: 64 profiles, tangent altitude h ~ U[3, 68] km, sorted by (profile, h).  A limb ray
has about 2 (z_top - h) / raydz points (raydz = 0.5 km), and its refraction probes -- 58 % of a tracer step's
instructions -- run only below 60 km, so a ray costs the tracer 0.42 np + 0.58 (points below 60 km); the look-up and the
radiance update np.  A workgroup costs what its longest ray costs.  The chip has `places` resident workgroups; a free
place takes the next workgroup of the hand-out order (a heap of finishing times).  Orders: slot order; the order of
jurk_block_order -- blocks of 256 slots ascending in the tangent altitude of their lowest ray, the parts of a block
adjacent --; the same keyed by the block's FIRST slot, which sends the 63 blocks that straddle two profiles (they begin
with the highest rays of one and hold the lowest of the next) to the end of the launch and is worse than slot order; and
as bounds the order by true cost and max(sum / places, longest workgroup).  Durations are fixed: on the
machine a wavefront on an emptier SIMD runs faster and the radiance update is bound by HBM, so the gains are upper
estimates.

usage: dispatch_order_model.py [rays [seed]]"""
import heapq
import sys
import numpy as np


def makespan(cost, places):
    free = [0.0] * places
    heapq.heapify(free)
    end = 0.0
    for c in cost:
        t = heapq.heappop(free) + c
        end = max(end, t)
        heapq.heappush(free, t)
    return end


def main():
    nr = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
    rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 0)
    prof = np.arange(nr) % 64
    h = rng.uniform(3.0, 68.0, nr)
    slot = np.lexsort((h, prof))
    h, prof = h[slot], prof[slot]
    nblk = (nr + 255) // 256
    hpad = np.full(nblk * 256, np.inf)
    hpad[:nr] = h
    first_order = np.argsort(h[::256], kind="stable")                # key: the block's first slot
    blk_order = np.argsort(hpad.reshape(nblk, 256).min(axis=1), kind="stable")   # key: the block's lowest ray
    straddle = int((prof[::256][:nblk] != prof[np.minimum(np.arange(nblk) * 256 + 255, nr - 1)]).sum())
    print("%d rays, %d blocks of 256 slots, %d of them straddle two profiles" % (nr, nblk, straddle))
    print("%-44s %9s %9s %9s %9s %9s" % ("launch (model units)", "in-order", "first ray", "blk_order", "by cost", "ideal"))

    def row(name, ray_cost, wg, places, items=1):
        n = (nr + wg - 1) // wg
        pad = np.zeros(n * wg)
        pad[:nr] = ray_cost
        cost = pad.reshape(n, wg).max(axis=1)
        m = 256 // wg                                                # workgroups to the block
        def by(order):
            o = (order[:, None] * m + np.arange(m)[None, :]).ravel()
            return cost[o[o < n]]
        rep = lambda c: np.repeat(c, items)                          # the `items` workgroups of a ray block are adjacent
        print("%-44s %9.0f %9.0f %9.0f %9.0f %9.0f" % (name, makespan(rep(cost), places), makespan(rep(by(first_order)), places),
                                                 makespan(rep(by(blk_order)), places),
                                                 makespan(rep(np.sort(cost)[::-1]), places),
                                                 max(cost.sum() * items / places, cost.max())))

    for ztop in (90.0, 120.0):
        npts = 2.0 * (ztop - h) / 0.5
        low = 2.0 * np.maximum(60.0 - h, 0.0) / 0.5
        row("tracer, z_top = %g km (256 rays, 1024 places)" % ztop, 0.42 * npts + 0.58 * low, 256, 1024)
    npts = 2.0 * (90.0 - h) / 0.5
    row("radiance update (128 rays, 1024 places)", npts, 128, 1024)
    row("look-up (256 rays x 20 pairs, 1792 places)", npts, 256, 1792, items=20)


if __name__ == "__main__":
    main()
