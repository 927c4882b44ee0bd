"""CPU restatement of the reference's prescribed-motion ADVECTION-diffusion blocks -- test infrastructure only.

  psip_conv / psim_conv                       /root/reference/src/prescribedmotionsolver/advectiondiffusion.jl:35-61
  MovingAdvDiffusionUnsteadyMono              .../advectiondiffusion.jl:15-33
  A_mono_unstead_advdiff_moving               .../advectiondiffusion.jl:64-129
  b_mono_unstead_advdiff_moving               .../advectiondiffusion.jl:131-199
  MovingAdvDiffusionUnsteadyDiph              .../advectiondiffusion.jl:246-264
  A_diph_unstead_advdiff_moving               .../advectiondiffusion.jl:266-386
  b_diph_unstead_advdiff_moving               .../advectiondiffusion.jl:388-507

Literal: the operator is `oracle.penguin_oracle.make_convection_ops` applied to the (N+1)-D space-time capacity (full
Kronecker operators of 2M rows), and the blocks slice it exactly as the reference does -- `C[1][L1,L1]`, `C[2][L2,L2]`,
`C[3][L1,L2]` and the same of K, `[1:end÷2]` of G, H, Wꜝ, V -- so that every quirk of those slices (no bulk y-advection, ½K_x
only) comes out of the algebra rather than being written in.  The moving-diffusion helpers of `oracle/spacetime.py` supply Ψ,
the half selections and the border rows.
"""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp

from oracle import penguin_oracle as po
from oracle import spacetime as ost

_half = ost._half


def psip_conv(a, b):
    if a == 0 and b == 0:
        return 0.0
    if a != 0 and b != 0:
        return 0.0
    if a == 0 and b != 0:          # "Fresh"
        return 1.0
    return 0.0                     # "Dead"


def psim_conv(a, b):
    if a == 0 and b == 0:
        return 0.0
    if a != 0 and b != 0:
        return 1.0
    if a == 0 and b != 0:          # "Fresh"
        return 0.0
    return 1.0                     # "Dead"


def _diag(fn, Vn, Vn_1):
    return sp.diags(np.array([fn(a, b) for a, b in zip(Vn, Vn_1)], dtype=float))


def convection_blocks(op: po.ConvectionOps):
    """`C = C[1][1:end÷2, 1:end÷2], C[2][end÷2+1:end, end÷2+1:end], C[3][1:end÷2, end÷2+1:end]` and the same of K (:94-95)."""
    def three(X):
        h = X[0].shape[0] // 2
        return X[0].tocsr()[:h, :h], X[1].tocsr()[h:, h:], X[2].tocsr()[:h, h:]
    return three(op.C), three(op.K)


def _time_faces(op, cap):
    At = cap.A[len(op.size) - 1]
    return At[: len(At) // 2], At[len(At) // 2:]


def A_mono_unstead_advdiff_moving(op: po.ConvectionOps, cap: po.Capacity, D, bc, scheme: str) -> sp.csr_matrix:
    """advectiondiffusion.jl:64-129."""
    Vn_1, Vn = _time_faces(op, cap)
    psip = ost.psip_cn if scheme == "CN" else ost.psip_be
    Psi = _diag(psip, Vn, Vn_1)
    Ia, Ib = po.build_I_bc(op, bc)
    Ig = _half(sp.diags(cap.G))
    Id = _half(sp.diags(po.build_I_D(op, D, cap)))
    C, K = convection_blocks(op)
    Wi, G, H = _half(op.Winv), _half(op.G), _half(op.H)
    Psi_conv = _diag(psip_conv, Vn, Vn_1)
    GT, HT = G.T.tocsr(), H.T.tocsr()
    sumC = C[0] + C[1] + C[2]
    block1 = sp.diags(Vn_1) + Id @ GT @ Wi @ G @ Psi - (sumC + 0.5 * K[0]) @ Psi_conv          # :123
    block2 = -(sp.diags(Vn_1) - sp.diags(Vn)) + Id @ GT @ Wi @ H @ Psi - 0.5 * K[0] @ Psi_conv   # :124
    block3 = Ib * (HT @ Wi @ G)
    block4 = Ib * (HT @ Wi @ H) + Ia * Ig
    return sp.bmat([[block1, block2], [block3, block4]], format="csr")


def b_mono_unstead_advdiff_moving(op, cap, D, f, bc, Ti, dt, t, scheme) -> np.ndarray:
    """advectiondiffusion.jl:131-199."""
    fn = po.build_source(op, f, t, cap)
    fn1 = po.build_source(op, f, t + dt, cap)
    gg = po.build_g_g(op, bc, cap)
    Id = _half(sp.diags(po.build_I_D(op, D, cap)))
    Vn_1, Vn = _time_faces(op, cap)
    psim = ost.psim_cn if scheme == "CN" else ost.psim_be
    Psin = _diag(psim, Vn, Vn_1)
    C, K = convection_blocks(op)
    Wi, G, H, V = _half(op.Winv), _half(op.G), _half(op.H), _half(op.V)
    Ig = _half(sp.diags(cap.G))
    To, Tg = Ti[: len(Ti) // 2], Ti[len(Ti) // 2:]
    fn, fn1, gg = _half(fn), _half(fn1), _half(gg)
    Psi_conv = _diag(psim_conv, Vn, Vn_1)
    GT = G.T.tocsr()
    sumC = C[0] + C[1] + C[2]
    if scheme == "CN":                                                                        # :192
        b1 = ((sp.diags(Vn) - Id @ GT @ Wi @ G @ Psin) @ To - 0.5 * (Id @ GT @ Wi @ H @ Tg) + 0.5 * (V @ (fn + fn1))
              - 0.5 * (K[0] @ (Psin @ To)) - 0.5 * (K[0] @ Tg) - sumC @ To)
    else:                                                                                     # :194
        b1 = Vn * To + V @ fn1 - 0.5 * (K[0] @ (Psi_conv @ To)) - 0.5 * (K[0] @ Tg) - sumC @ (Psi_conv @ To)
    b2 = Ig @ gg                                                                              # :196
    return np.concatenate([b1, b2])


def MovingAdvDiffusionUnsteadyMono(phase: po.Phase, bc_b, bc_i, dt, Ti, mesh: po.Mesh, scheme: str) -> po.Solver:
    """advectiondiffusion.jl:15-33 (t = 0.0 in b and in the border rows)."""
    s = po.Solver("Unsteady", "Monophasic", "DiffusionAdvection")
    sch = "CN" if scheme == "CN" else "BE"
    s.A = A_mono_unstead_advdiff_moving(phase.operator, phase.capacity, phase.Diffusion_coeff, bc_i, sch)
    s.b = b_mono_unstead_advdiff_moving(phase.operator, phase.capacity, phase.Diffusion_coeff, phase.source, bc_i, Ti, dt, 0.0, sch)
    s.A, s.b = po.BC_border_mono(s.A, s.b, bc_b, mesh, t=0.0)
    return s


def A_diph_unstead_advdiff_moving(op1, op2, cap1, cap2, D1, D2, ic: po.InterfaceConditions, scheme: str) -> sp.csr_matrix:
    """advectiondiffusion.jl:266-386."""
    jump, flux = ic.scalar, ic.flux
    Vn1_1, Vn1 = _time_faces(op1, cap1)
    Vn2_1, Vn2 = _time_faces(op2, cap2)
    psip = ost.psip_cn if scheme == "CN" else ost.psip_be
    Psi1, Psi2 = _diag(psip, Vn1, Vn1_1), _diag(psip, Vn2, Vn2_1)
    n = len(Vn1)
    Ia1, Ia2 = jump.alpha1 * sp.identity(n), jump.alpha2 * sp.identity(n)
    Ib1, Ib2 = flux.beta1, flux.beta2
    C1, K1 = convection_blocks(op1)
    C2, K2 = convection_blocks(op2)
    W1, G1, H1 = _half(op1.Winv), _half(op1.G), _half(op1.H)
    W2, G2, H2 = _half(op2.Winv), _half(op2.G), _half(op2.H)
    Id1, Id2 = _half(sp.diags(po.build_I_D(op1, D1, cap1))), _half(sp.diags(po.build_I_D(op2, D2, cap2)))
    Pc1, Pc2 = _diag(psip_conv, Vn1, Vn1_1), _diag(psip_conv, Vn2, Vn2_1)
    G1T, H1T, G2T, H2T = G1.T.tocsr(), H1.T.tocsr(), G2.T.tocsr(), H2.T.tocsr()
    sC1, sC2 = C1[0] + C1[1] + C1[2], C2[0] + C2[1] + C2[2]
    block1 = sp.diags(Vn1_1) + Id1 @ G1T @ W1 @ G1 @ Psi1 - (sC1 + 0.5 * K1[0]) @ Pc1            # :357
    block2 = -(sp.diags(Vn1_1) - sp.diags(Vn1)) + Id1 @ G1T @ W1 @ H1 @ Psi1 - 0.5 * K1[0] @ Pc1
    block3 = sp.diags(Vn2_1) + Id2 @ G2T @ W2 @ G2 @ Psi2 - (sC2 + 0.5 * K2[0]) @ Pc2
    block4 = -(sp.diags(Vn2_1) - sp.diags(Vn2)) + Id2 @ G2T @ W2 @ H2 @ Psi2 - 0.5 * K2[0] @ Pc2
    block5 = Ib1 * (H1T @ W1 @ G1 @ Psi1)                                                       # :362-365: no -(Vn_1 - Vn)
    block6 = Ib1 * (H1T @ W1 @ H1 @ Psi1)
    block7 = Ib2 * (H2T @ W2 @ G2 @ Psi2)
    block8 = Ib2 * (H2T @ W2 @ H2 @ Psi2)
    Z = sp.csr_matrix((n, n))
    return sp.bmat([[block1, block2, Z, Z], [Z, Ia1, Z, -Ia2], [Z, Z, block3, block4], [block5, block6, block7, block8]], format="csr")


def b_diph_unstead_advdiff_moving(op1, op2, cap1, cap2, D1, D2, f1, f2, ic: po.InterfaceConditions, Ti, dt, t, scheme) -> np.ndarray:
    """advectiondiffusion.jl:388-507."""
    jump, flux = ic.scalar, ic.flux
    f1n, f1n1 = po.build_source(op1, f1, t, cap1), po.build_source(op1, f1, t + dt, cap1)
    f2n, f2n1 = po.build_source(op2, f2, t, cap2), po.build_source(op2, f2, t + dt, cap2)
    gg = po.build_g_g(op1, jump, cap1)
    hh = po.build_g_g(op2, flux, cap2)
    Vn1_1, Vn1 = _time_faces(op1, cap1)
    Vn2_1, Vn2 = _time_faces(op2, cap2)
    psim = ost.psim_cn if scheme == "CN" else ost.psim_be
    Psi1, Psi2 = _diag(psim, Vn1, Vn1_1), _diag(psim, Vn2, Vn2_1)
    C1, K1 = convection_blocks(op1)
    C2, K2 = convection_blocks(op2)
    q = len(Ti) // 4
    To1, Tg1, To2, Tg2 = Ti[:q], Ti[q:2 * q], Ti[2 * q:3 * q], Ti[3 * q:]
    f1n, f1n1, f2n, f2n1 = _half(f1n), _half(f1n1), _half(f2n), _half(f2n1)
    gg, hh = _half(gg), _half(hh)
    Ig2 = _half(sp.diags(cap2.G))
    Id1, Id2 = _half(sp.diags(po.build_I_D(op1, D1, cap1))), _half(sp.diags(po.build_I_D(op2, D2, cap2)))
    W1, G1, H1, V1 = _half(op1.Winv), _half(op1.G), _half(op1.H), _half(op1.V)
    W2, G2, H2, V2 = _half(op2.Winv), _half(op2.G), _half(op2.H), _half(op2.V)
    Pc1, Pc2 = _diag(psim_conv, Vn1, Vn1_1), _diag(psim_conv, Vn2, Vn2_1)
    G1T, G2T = G1.T.tocsr(), G2.T.tocsr()
    sC1, sC2 = C1[0] + C1[1] + C1[2], C2[0] + C2[1] + C2[2]
    if scheme == "CN":                                                                          # :494-495
        b1 = ((sp.diags(Vn1) - Id1 @ G1T @ W1 @ G1 @ Psi1) @ To1 - 0.5 * (Id1 @ G1T @ W1 @ H1 @ Tg1) + 0.5 * (V1 @ (f1n + f1n1))
              - sC1 @ To1 - 0.5 * (K1[0] @ To1) - 0.5 * (K1[0] @ Tg1))
        b3 = ((sp.diags(Vn2) - Id2 @ G2T @ W2 @ G2 @ Psi2) @ To2 - 0.5 * (Id2 @ G2T @ W2 @ H2 @ Tg2) + 0.5 * (V2 @ (f2n + f2n1))
              - sC2 @ To2 - 0.5 * (K2[0] @ To2) - 0.5 * (K2[0] @ Tg2))
    else:                                                                                       # :497-498
        b1 = Vn1 * To1 + V1 @ f1n1 - 0.5 * (K1[0] @ (Pc1 @ To1)) - 0.5 * (K1[0] @ Tg1) - sC1 @ (Pc1 @ To1)
        b3 = Vn2 * To2 + V2 @ f2n1 - 0.5 * (K2[0] @ (Pc2 @ To2)) - 0.5 * (K2[0] @ Tg2) - sC2 @ (Pc2 @ To2)
    b2 = gg                                                                                     # :502 (no Γ)
    b4 = Ig2 @ hh
    return np.concatenate([b1, b2, b3, b4])


def MovingAdvDiffusionUnsteadyDiph(phase1: po.Phase, phase2: po.Phase, bc_b, ic, dt, Ti, mesh: po.Mesh, scheme: str) -> po.Solver:
    """advectiondiffusion.jl:246-264 (t = 0.0 in b; BC_border_diph! without t)."""
    s = po.Solver("Unsteady", "Diphasic", "DiffusionAdvection")
    sch = "CN" if scheme == "CN" else "BE"
    s.A = A_diph_unstead_advdiff_moving(phase1.operator, phase2.operator, phase1.capacity, phase2.capacity, phase1.Diffusion_coeff,
                                        phase2.Diffusion_coeff, ic, sch)
    s.b = b_diph_unstead_advdiff_moving(phase1.operator, phase2.operator, phase1.capacity, phase2.capacity, phase1.Diffusion_coeff,
                                        phase2.Diffusion_coeff, phase1.source, phase2.source, ic, Ti, dt, 0.0, sch)
    s.A, s.b = ost._border_diph(s.A, s.b, bc_b, phase1.capacity, phase2.capacity, mesh, None)
    return s
