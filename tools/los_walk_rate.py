"""los.LOSFieldSampler: steps and thetas per second of the device ensemble sampler over a field of
sightlines, beside the same loop written with torch ops and beside the host form, in the same run
on the same machine.  Needs a GPU:

    python tools/los_walk_rate.py [--reps 5] [--steps 20] [--host-sightlines 4] [--out FILE]

Workload A: 1000 synthetic sightlines x 200 stars x 25 draws, 4 clouds, W = 32 walkers.
Workload B: 10 000 sightlines x 50 stars.  A step moves every walker once: S x W thetas.
  sampler     `LOSFieldSampler.run(steps, device_out=True)`, one synchronisation per timed run
  torch ops   what a user can write without it: the stretch move with torch's generator, the
              prior transform with `torch.special.ndtri`, `torch.sort` / `gather` for the clouds
              and `F(tensor, device_out=True)` for the likelihood; the same synchronisation
  host form   `LOS_walk_field_host` over the first `--host-sightlines` sightlines (the time of
              `--host-steps` + 1 steps less that of 1), scaled to the field by the number of
              sightlines (it is a loop over them): an extrapolation
A figure is the median of `--reps` timed runs after a warm-up run, with the spread (min .. max).
The kernel times are HIP events (brutus_enable_timing) summed over the half-steps of
`--steps` steps; the share of the walk kernels is theirs of that sum.  Writes
profiles/los_walk_rate.txt."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from brutus_amd import _lib, los  # noqa: E402
from los_rate import kernel_times, sightline  # noqa: E402

NCLOUDS, W = 4, 32


def spread(fn, reps, per_run):
    """`per_run` / seconds of `fn()`: median, min, max over `reps` runs after a warm-up run."""
    out = []
    for _ in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(per_run / (time.perf_counter() - t0))
    return np.median(out[1:]), min(out[1:]), max(out[1:])


class TorchWalk(object):
    """The sampler's algorithm in torch ops over `F(tensor, device_out=True)`."""

    def __init__(self, F, prior, u0):
        self.F, self.P = F, prior
        self.u = torch.from_numpy(u0).to(F.device)
        self.gen = torch.Generator(device=F.device)
        self.gen.manual_seed(1)
        self.lnl = F(self.transform(self.u), device_out=True)

    def lognormal(self, q, params):
        mean, std, low, high = params
        a, b = (low - mean) / std, (high - mean) / std
        cdf = lambda x: float(torch.special.ndtr(torch.tensor(x, dtype=torch.float64)))
        p = cdf(a) + q * (cdf(b) - cdf(a))
        lower = torch.special.ndtri(p.clamp(max=0.5))
        upper = -torch.special.ndtri((cdf(-b) + (1. - q) * (cdf(-a) - cdf(-b))).clamp(max=0.5))
        return torch.exp((mean + std * torch.where(p <= 0.5, lower, upper)).clamp(low, high))

    def transform(self, u):
        P = self.P
        th = torch.empty_like(u)
        th[..., 0] = self.lognormal(u[..., 0], P.pb_params)
        th[..., 1:3] = self.lognormal(u[..., 1:3], P.s_params)
        th[..., 3] = u[..., 3] * (P.rlims[1] - P.rlims[0]) + P.rlims[0]
        d, order = torch.sort(u[..., 4::2], dim=-1, stable=True)
        th[..., 4::2] = d * (P.dlims[1] - P.dlims[0]) + P.dlims[0]
        th[..., 5::2] = torch.gather(u[..., 5::2], -1, order) * (P.rlims[1] - P.rlims[0]) + P.rlims[0]
        return th

    def step(self):
        u, lnl = self.u, self.lnl
        S, nw, ncol = u.shape
        for half in (0, 1):
            r = torch.rand((3, S, nw // 2), generator=self.gen, device=u.device, dtype=torch.float64)
            z = (r[0] + 1.) ** 2 / 2.
            j = (r[1] * (nw // 2)).floor().long()
            uw, uo = u[:, half::2], u[:, 1 - half::2]
            uj = torch.gather(uo, 1, j[..., None].expand(-1, -1, ncol))
            un = uj + z[..., None] * (uw - uj)
            inside = ((un >= 0.) & (un <= 1.)).all(dim=-1)
            ln = self.F(self.transform(un.clamp(0., 1.)), device_out=True)
            acc = inside & (r[2].log() < (ncol - 1) * z.log() + ln - lnl[:, half::2])
            u[:, half::2] = torch.where(acc[..., None], un, uw)
            lnl[:, half::2] = torch.where(acc, ln, lnl[:, half::2])


def kernel_share(S, L, steps):
    """ms per kernel summed over the half-steps of `steps` steps, with the library's timers on."""
    tot = {}
    L.brutus_enable_timing(1)

    def after(_):
        for name, ms in kernel_times(L):
            tot[name] = tot.get(name, 0.) + ms
    with torch.cuda.device(S.field.device):
        stream = torch.cuda.current_stream().cuda_stream
        S.field._buffers(S.nwalkers // 2, S.nparams)
        for g in range(S.step, S.step + steps):
            for half in (0, 1):
                S._half_step(g, half, None, None, stream, after)
    S.step += steps
    L.brutus_enable_timing(0)
    return tot


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--host-sightlines", type=int, default=4)
    ap.add_argument("--host-steps", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "los_walk_rate.txt"))
    a = ap.parse_args()
    L = _lib.lib()
    prior = los.LOSPrior()
    lines = ["los.LOSFieldSampler, steps and thetas per second (a step = S x W thetas; W = %d, %d clouds, gauss, "
             "25 draws)" % (W, NCLOUDS),
             "(median of %d runs of %d steps after a warm-up run; min .. max)" % (a.reps, a.steps),
             torch.cuda.get_device_name(0), ""]
    for label, nsight, nobj in (("A", 1000, 200), ("B", 10000, 50)):
        pairs = [sightline(nobj, 25, 1000 * nobj + s) for s in range(nsight)]
        F = los.LOSField(pairs)
        S = los.LOSFieldSampler(F, prior, W, seed=1, nclouds=NCLOUDS)
        per_step = nsight * W
        dev = spread(lambda: S.run(a.steps, thin=a.steps, device_out=True), a.reps, a.steps)
        T = TorchWalk(F, prior, los._walk_start(1, np.arange(nsight), W, NCLOUDS, True))
        tor = spread(lambda: [T.step() for _ in range(a.steps)], a.reps, a.steps)
        nh = min(a.host_sightlines, nsight)
        took = []
        for n in (1, 1 + a.host_steps):                 # (the difference leaves the first state out)
            t0 = time.perf_counter()
            los.LOS_walk_field_host(pairs[:nh], prior, W, n, seed=1, nclouds=NCLOUDS)
            took.append(time.perf_counter() - t0)
        host = a.host_steps / (took[1] - took[0]) * nh / nsight
        tot = kernel_share(S, L, a.steps)
        walk = sum(ms for name, ms in tot.items() if name.startswith("k_los_walk"))
        row = ["workload %s: %d sightlines x %d stars" % (label, nsight, nobj),
               "    sampler, device                 %10.2f steps/s (%.2f .. %.2f) = %.3g thetas/s"
               % (dev + (dev[0] * per_step,)),
               "    torch ops on F(device_out=True) %10.2f steps/s (%.2f .. %.2f) = %.3g thetas/s"
               % (tor + (tor[0] * per_step,)),
               "    host form, EXTRAPOLATED from %d sightlines x %d steps: %.4f steps/s = %.3g thetas/s"
               % (nh, a.host_steps, host, host * per_step),
               "    sampler / torch ops = %.2f, sampler / host form = %.0f" % (dev[0] / tor[0], dev[0] / host),
               "    kernels of %d steps, ms: " % a.steps + ", ".join("%s %.3f" % kv for kv in sorted(tot.items())),
               "    share of the two walk kernels: %.1f %% of the kernel time of a step"
               % (100. * walk / sum(tot.values())), ""]
        lines += row
        print("\n".join(row), flush=True)
        del F, S, T
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
