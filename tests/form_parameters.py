"""Case tables of the form-parameter tests (tests/test_form_parameters_host.py on the CPU oracle,
tests/test_gpu_form_parameters.py on the device): Poisson ratios on both sides of the uniform-nu
kernels' interval, and quadrature degrees other than each element's default. Tables only.

The Poisson ratios follow csrc/femasm.hip: lin_uniform_nu() sends a linear-elasticity form with E per
cell to the uniform-nu kernels (MAT_LINU, MAT_AFFT, k_gather_lin, the prepared state with k_cell_coef)
for  -0.99 < nu < 0.49  (both comparisons strict), and to the general lam/mu kernels outside. A change
of those thresholds is made here too: NU holds each threshold and its nearest inside neighbour.
nu = 0.5, nu = -1 and anything beyond have no finite Lame parameters and stay out."""

TRI, QUAD, TET, HEX = 3, 4, -4, 8

NU_LO, NU_HI = -0.99, 0.49  # lin_uniform_nu(): uniform-nu kernels for NU_LO < nu < NU_HI
NU = [0.0, 0.2, 0.45, 0.4899, 0.49, 0.4999, -0.5, -0.9899, -0.99]
NU_SHORT = [0.0, 0.4899, 0.4999, -0.5]


def uniform_nu(nu: float) -> bool:
    """Whether lin_uniform_nu() takes this ratio (given E per cell and the linear law)."""
    return NU_LO < nu < NU_HI


# id -> (cell type, degree, cells per axis): the smallest meshes test_gpu_parity.CASES trusts
ELEMENTS = {
    "tri-P1": (TRI, 1, (8, 7)), "tri-P2": (TRI, 2, (5, 4)),
    "quad-Q1": (QUAD, 1, (5, 4)), "quad-Q2": (QUAD, 2, (4, 5)), "quad-Q3": (QUAD, 3, (3, 2)),
    "tet-P1": (TET, 1, (3, 4, 2)), "tet-P2": (TET, 2, (3, 2, 3)),
    "hex-Q1": (HEX, 1, (3, 2, 2)), "hex-Q2": (HEX, 2, (2, 2, 2)), "hex-Q3": (HEX, 3, (2, 1, 2)),
}
# the same meshes with their interior vertices moved by PERTURB * h (test_gpu_parity.test_non_affine_cells):
# trilinear hexahedra reach k_hex_mfma, bilinear quadrilaterals the generic kernels
NON_AFFINE = ["quad-Q1", "quad-Q2", "hex-Q1", "hex-Q2"]
PERTURB = 0.3
# (element id, perturb) of every matrix case
MESHES = [(e, 0.0) for e in ELEMENTS] + [(e, PERTURB) for e in NON_AFFINE]

# Non-default quadrature degrees per element (defaults: 2 (p - 1) on simplices, at least 1; 2 p on
# tensor cells): an under-integrating rule where there is one, and one or two richer rules. The largest
# rule (hex, degree 8) has 125 points; the oracle's static rule arrays hold ORA_MAXQ = 256.
QDEG = {
    "tri-P1": [2, 4], "tri-P2": [1, 4], "tet-P1": [2], "tet-P2": [1, 3, 4],
    "quad-Q1": [1, 4], "quad-Q2": [2, 6], "quad-Q3": [4, 8],
    "hex-Q1": [1, 4], "hex-Q2": [2, 6], "hex-Q3": [4, 8],
}
QDEG_CASES = [(e, q) for e, qs in QDEG.items() for q in qs]


def default_qdeg(ct: int, p: int) -> int:
    return max(2 * (p - 1), 1) if ct in (TRI, TET) else 2 * p


# residual cases: test_gpu_vector.CASES plus the Q3 elements, which no residual test ran before
VECTOR_CASES = {
    "tri-P1": (TRI, 1, (6, 5)), "tri-P2": (TRI, 2, (4, 3)), "quad-Q1": (QUAD, 1, (4, 3)), "quad-Q2": (QUAD, 2, (3, 3)),
    "tet-P1": (TET, 1, (2, 3, 2)), "tet-P2": (TET, 2, (2, 2, 2)), "hex-Q1": (HEX, 1, (2, 2, 2)),
    "hex-Q2": (HEX, 2, (2, 1, 2)), "quad-Q3": (QUAD, 3, (2, 2)), "hex-Q3": (HEX, 3, (1, 1, 2)),
}
Q3 = ["quad-Q3", "hex-Q3"]

# neo-Hookean and damage cases
NEO = {"tet-P2": (TET, 2, (3, 2, 3)), "tri-P2": (TRI, 2, (5, 4)), "hex-Q1": (HEX, 1, (3, 2, 2))}
NEO_QDEG = [("tet-P2", 1), ("tet-P2", 3), ("tet-P2", 4), ("tri-P2", 4), ("hex-Q1", 4)]
DAMAGE = (TRI, 1, (8, 7))

# deterministic=True: the elements the fixed-point gather serves (all on affine cells)
DETERMINISTIC = ["tri-P1", "tri-P2", "tet-P1", "tet-P2", "quad-Q1", "quad-Q2", "hex-Q1"]
# Jacobian action: planned kernels, and two elements of the generic one
OPERATOR = ["tri-P1", "tri-P2", "tet-P1", "tet-P2", "quad-Q2", "hex-Q1"]
