"""femasm — MI355X-native element-stiffness assembly (the hot path of SalzmanA/fem-libraries).

Submodules mirror the reference's dolfinx surface: ``mesh`` (meshes in torch tensors),
``fem`` (function spaces, forms, Dirichlet BCs, create_matrix / assemble_matrix, and the damage field built
from tagged entities: ``mark_vertices``, ``spread``, ``damage_field`` on ``mesh.vertex_graph``), ``la``
(the BSR global matrix), ``io`` (XDMF meshes and mesh tags), ``mg`` (geometric multigrid
preconditioner for ``nls.KrylovSolver``), ``geometry`` (point location: ``bb_tree``, ``locate_points``). Numerics run in libfemasm.so
(hand-written HIP for gfx950).
"""
from . import fem, geometry, io, la, mesh, mg  # noqa: F401
from ._lib import FemasmError, load  # noqa: F401

__version__ = "0.1.0"
