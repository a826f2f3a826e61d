"""SVGD against planar-flow VI on the 2-D energy potentials U1-U4.

Planar VI with K = 8 from the reference initialisation (W = U = b = 0.1, RMSProp) and Stein
variational gradient descent (RBF kernel, median bandwidth, Adam) are run on each potential and
compared by the kernel Stein discrepancy (IMQ, h = 1, U-statistic), which needs no normaliser and
so also covers U3 and U4. The free energy F exists for the flow only. On U1 the flow covers one
of the two modes from this initialisation (KL ~ log 2) while the particles cover both.

    python examples/svgd_potentials.py [--device cuda] [--iters 5000] [--svgd-iters 500]
    python examples/svgd_potentials.py --reduced        # seconds, the test mode
"""
from _common import outdir, parser, report

import torch

from vi_normflows_amd.distributions.energies import get_target
from vi_normflows_amd.inference.flow_vi import FlowVI, fit_flow_vi
from vi_normflows_amd.inference.svgd import fit_svgd, flow_ksd


def main(argv=None):
    ap = parser(__doc__, 5000, "svgd_potentials")
    ap.add_argument("--targets", default="U1,U2,U3,U4")
    ap.add_argument("--K", type=int, default=8)
    ap.add_argument("--lr", type=float, default=1e-2)
    ap.add_argument("--samples", type=int, default=100)
    ap.add_argument("--svgd-iters", type=int, default=500)
    ap.add_argument("--svgd-lr", type=float, default=0.05)
    ap.add_argument("--particles", type=int, default=1000)
    ap.add_argument("--reduced", action="store_true", help="tiny settings (the test mode)")
    a = ap.parse_args(argv)
    if a.reduced:
        a.iters, a.svgd_iters, a.particles = 60, 30, 100
    out = outdir(a.out)
    rows = {}
    for name in a.targets.split(","):
        # U2 without the reference's 1e7 gate outside |z1| <= 4: a single sample out there
        # would swamp F, and the gate has no gradient for either method to follow
        tgt = get_target(name, gate=False) if name.lower() in ("u2", "p2") else get_target(name)
        r = fit_flow_vi(tgt, "planar", a.K, a.iters, a.lr, a.samples, "rmsprop", device=a.device,
                        seed=a.seed, log_every=max(a.iters, 1))
        model = FlowVI(r.target, r.flow).to(a.device)
        g = torch.Generator(device=a.device).manual_seed(a.seed + 1)
        ksd_flow = float(flow_ksd(model, a.particles, g))
        sv = fit_svgd(tgt, a.particles, a.svgd_iters, a.svgd_lr, device=a.device, seed=a.seed,
                      log_every=0)
        z = sv.particles
        rows[name] = {"F_planar": r.final["free_energy"], "ksd_planar": ksd_flow,
                      "ksd_svgd": sv.history[-1]["ksd"], "ksd_svgd_init": sv.history[0]["ksd"],
                      "svgd_share_z1_pos": float((z[:, 0] > 0).float().mean())}
    print(f"{'target':8s} {'F planar':>10s} {'KSD planar':>12s} {'KSD SVGD':>12s}")
    for name, v in rows.items():
        print(f"{name:8s} {v['F_planar']:10.4f} {v['ksd_planar']:12.5f} {v['ksd_svgd']:12.5f}")
    return report(out, {"K": a.K, "particles": a.particles, "device": a.device, "targets": rows})


if __name__ == "__main__":
    main()
