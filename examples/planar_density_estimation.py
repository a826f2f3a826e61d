"""Maximum-likelihood density estimation with a planar flow.

Samples are drawn from the known flow of ``learning_basic_flow`` (a 2-D standard normal pushed
through the planar layer w = [-5, 1], u = [-2, 1], b = 0). A ``PlanarStack`` is then fit to the
samples alone by maximising their likelihood: ``FlowDistribution.log_prob`` inverts the stack
(the fused inverse kernel on a GPU), so the loss is the exact negative log-likelihood rather than
a free energy against a known target. The held-out NLL is printed next to the exact NLL of the
same points under the true density (``planar_pushforward``), the floor no model can beat in
expectation.

    python examples/planar_density_estimation.py [--K 1] [--iters 600] [--train 4000]
"""
from _common import outdir, parser, report

import torch

from vi_normflows_amd.distributions.base import StdNormal
from vi_normflows_amd.distributions.energies import planar_pushforward
from vi_normflows_amd.flows import FlowDistribution, PlanarStack
from vi_normflows_amd.flows.planar import planar_stack_reference
from vi_normflows_amd.inference.flow_vi import fit_density

W_TRUE, U_TRUE, B_TRUE = (-5.0, 1.0), (-2.0, 1.0), 0.0


def known_flow_samples(n, generator=None, dtype=torch.float64):
    """n draws of y = z + u_hat tanh(w.z + b), z ~ N(0, I)."""
    z = torch.randn(n, 2, generator=generator, dtype=dtype)
    W = torch.tensor([W_TRUE], dtype=dtype)
    U = torch.tensor([U_TRUE], dtype=dtype)
    return planar_stack_reference(z, W, U, torch.tensor([B_TRUE], dtype=dtype))[0]


def main(argv=None):
    ap = parser(__doc__, 600, "planar_density")
    ap.add_argument("--K", type=int, default=1)
    ap.add_argument("--train", type=int, default=4000)
    ap.add_argument("--heldout", type=int, default=2000)
    ap.add_argument("--lr", type=float, default=0.02)
    a = ap.parse_args(argv)
    out = outdir(a.out)
    dev = torch.device(a.device)
    dtype = torch.float32 if dev.type == "cuda" else torch.float64
    g = torch.Generator().manual_seed(a.seed)
    train = known_flow_samples(a.train, g).to(dev, dtype)
    held = known_flow_samples(a.heldout, g).to(dev, dtype)
    exact_nll = float(-planar_pushforward(W_TRUE, U_TRUE, B_TRUE)(held).mean())
    flow = PlanarStack(2, a.K, init="random", generator=g).to(dev, dtype)
    dist = FlowDistribution(StdNormal(2), flow)
    with torch.no_grad():
        nll0 = float(-dist.log_prob(held).mean())
    trace = fit_density(flow, train, iters=a.iters, lr=a.lr)
    with torch.no_grad():
        nll = float(-dist.log_prob(held).mean())
    print(f"held-out NLL {nll0:.4f} -> {nll:.4f}   exact NLL {exact_nll:.4f}")
    if not a.no_plots:
        from vi_normflows_amd.viz import plot_flow_density, plot_loss

        plot_flow_density(dist, lims=(-8, 8), n=200, path=out / "density.png",
                          title=f"planar K={a.K}, maximum likelihood")
        plot_loss(trace, path=out / "nll.png", ylabel="training NLL")
    return report(out, {"K": a.K, "heldout_nll_init": nll0, "heldout_nll": nll,
                        "exact_nll": exact_nll, "train_nll": trace[-1] if trace else None,
                        "W": flow.W.detach().tolist(), "U_hat": flow.uhat().detach().tolist(),
                        "B": flow.B.detach().tolist()})


if __name__ == "__main__":
    main()
