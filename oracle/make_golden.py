#!/usr/bin/env python3
"""Record the reference implementation's results as fixtures under ``tests/golden/``.

The parity tests compare this package with the original NumPy ``normflows`` project. A checkout
of that project is not part of this repository, so its functions are run ONCE here, on the
fixed seeded inputs the tests regenerate, and only their numerical results are stored
(``tests/golden/reference_outputs.npz``). The data files the tests and examples read (the
linear-regression CSV, the shipped MNIST checkpoints, the free-energy logs) are copied as they
are. Nothing of the reference's program text is stored.

    python oracle/make_golden.py --reference /path/to/reference/checkout

Needs scipy (the reference's densities use it). Re-running reproduces the committed files.
"""
from __future__ import annotations

import argparse
import shutil
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden"
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(Path(__file__).resolve().parent))   # ref_shim.py

DATA_FILES = ["data/HW0_data.csv", "results/free_energy.txt", "results/free_energy2d.txt",
              "results/reg_free_energy2d.txt"]


def _arch(Din, H, L, Dout, act, out_act=None):
    a = {"width": H, "hidden_layers": L, "input_dim": Din, "output_dim": Dout,
         "activation_fn_type": "relu", "activation_fn_params": "", "activation_fn": act}
    if out_act:
        a["output_activation_fn"] = out_act
    return a


def copy_data(ref: Path) -> None:
    files = [ref / f for f in DATA_FILES] + sorted((ref / "models").glob("*/*.npy"))
    for src in files:
        dst = GOLDEN / src.relative_to(ref)
        dst.parent.mkdir(parents=True, exist_ok=True)
        shutil.copyfile(src, dst)
        dst.chmod(0o644)


def record(ref: Path) -> dict:
    from ref_shim import load_defs, ref_module

    from vi_normflows_amd.models.vae import synthetic_binary_images
    from vi_normflows_amd.utils.npy_io import load_flat

    out = {}
    relu = lambda x: np.maximum(x, 0)  # noqa: E731
    sig = lambda x: 1 / (1 + np.exp(-x))  # noqa: E731

    # tests/test_models_compat.py::test_feedforward_matches_reference_forward
    rnn = ref_module(ref, "nn_models")
    net = rnn.Feedforward(_arch(5, 7, 3, 4, relu))
    rng = np.random.RandomState(0)
    W = rng.randn(3, net.D)
    x = rng.randn(5, 11)
    out["ff_D"] = np.array(net.D)
    out["ff_forward"] = net.forward(W, x)
    xs = rng.randn(3, 5, 11)
    out["ff_forward_batched"] = net.forward(W, xs)
    out["ff_forward_first"] = net.forward(W[:1], x)[0]

    # tests/test_models_compat.py::test_vae_decodes_reference_checkpoint_like_reference
    rflows = ref_module(ref, "flows")
    K, dz = 2, 2
    phi = load_flat(ref / "models" / "reg_mnist" / f"weights_phi_{K}.npy")
    theta = load_flat(ref / "models" / "reg_mnist" / f"weights_theta_{K}.npy")
    enc = rnn.Feedforward(_arch(784, 64, 3, 2 * dz + 2 * dz * K + K, relu))
    dec = rnn.Feedforward(_arch(dz, 64, 3, 784, relu, sig))
    x = synthetic_binary_images(1, seed=3).numpy().astype(np.float64)
    P = enc.forward(phi.reshape(1, -1), x.T)[0]
    mu0, lsd = P[:dz].reshape(1, dz), P[dz:2 * dz].reshape(1, dz)
    Wf = P[2 * dz:2 * dz + K * dz].reshape(K, 1, dz)
    Uf = P[2 * dz + K * dz:2 * dz + 2 * K * dz].reshape(K, 1, dz)
    bf = P[-K:].reshape(K, 1)
    eps = np.random.RandomState(0).randn(1, dz)
    z = eps * np.sqrt(1e-7 + np.exp(lsd)) + mu0
    for k in range(K):
        z = rflows.planar_flow(z, Wf[k], Uf[k], bf[k])
    out["vae_x"] = x
    out["vae_probs"] = dec.forward(theta.reshape(1, -1), z.T)[0].T

    # tests/test_flows.py::test_planar_matches_reference_source
    rng = np.random.RandomState(0)
    N, D = 7, 3
    z, w, u, b = rng.randn(N, D), rng.randn(N, D), rng.randn(N, D), rng.randn(N)
    out["planar_flow"] = rflows.planar_flow(z, w, u, b)
    out["planar_uhat"] = rflows._get_uhat(u, w)
    out["planar_m_0p3"] = np.array(float(rflows.m(0.3)))

    # tests/test_distributions_targets.py::test_log_mvn_matches_reference_for_D_ge_2_and_fixes_Q5
    refd = ref_module(ref, "distributions")
    rng = np.random.RandomState(0)
    Z, mu, lv = rng.randn(6, 3), rng.randn(1, 3), rng.randn(3)
    out["log_mvn_3d"] = refd.log_mvn(Z, mu, lv)
    Z1, lv1 = rng.randn(5, 1), np.array([0.3])
    out["log_mvn_1d"] = refd.log_mvn(Z1, np.zeros((1, 1)), lv1)

    # tests/test_distributions_targets.py::test_std_norm_mvn_gmm_bernoulli_match_reference
    rng = np.random.RandomState(1)
    x = rng.randn(7, 4)
    out["log_std_norm"] = refd.log_std_norm(x)
    Z = rng.randn(5, 1)
    out["mvn_1d"] = refd.mvn(Z, np.array([0.5]), np.array([2.0]))
    cov = np.array([[2.0, 0.3], [0.3, 1.0]])
    Z2 = rng.randn(5, 2)
    out["mvn_2d"] = refd.mvn(Z2, np.array([0.1, -0.2]), cov)
    mus, sg, pi = np.array([[0.0], [4.0]]), np.array([[1.0], [1.0]]), np.array([0.3])
    xx = np.linspace(-3, 8, 50).reshape(-1, 1)
    out["prob_gm"] = refd.prob_gm(xx, mus, sg, pi)
    lsd, lpi = np.log(sg), np.array([0.2])
    out["log_prob_gm"] = refd.log_prob_gm(xx, mus, lsd, lpi)
    X = (rng.rand(4, 10) > 0.5).astype(float)
    p = rng.rand(4, 10)
    out["log_bern_mult"] = np.array(refd.log_bern_mult(X, p))

    # tests/test_distributions_targets.py::test_targets_match_reference_get_data / gmm1d
    ns = load_defs(str(ref / "get_data.py"))
    for name in ("p1", "p2", "p3", "p4", "trial1"):
        z = np.random.RandomState(2).randn(200, 2) * 1.5
        out[f"target_{name}"] = ns[name](z)
    out["target_gmm"] = ns["gmm"](np.linspace(-5, 7, 101))
    return {k: np.asarray(v, dtype=np.float64) for k, v in out.items()}


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--reference", required=True, help="checkout of the reference project")
    a = ap.parse_args()
    ref = Path(a.reference)
    GOLDEN.mkdir(parents=True, exist_ok=True)
    copy_data(ref)
    np.savez(GOLDEN / "reference_outputs.npz", **record(ref))


if __name__ == "__main__":
    main()
