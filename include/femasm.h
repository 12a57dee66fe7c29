/*
 * femasm — MI355X (gfx950) element-stiffness assembly, C ABI.
 *
 * The drop-in boundary for the reference's hot path (SalzmanA/fem-libraries, mechanic2d):
 * the per-cell B^T.D.B quadrature contraction and its scatter into a global sparse matrix.
 * All pointers are DEVICE pointers (hipMalloc / torch.cuda tensors) unless stated; every
 * call is asynchronous on `stream` (a hipStream_t; NULL = the default stream) unless it
 * returns a size the host needs, which is stated per function.  Buffers are owned by the
 * caller; the library allocates only stream-ordered scratch that it frees before returning.
 * Errors: every function returns FA_OK (0) or a negative FA_E_* code and sets a
 * thread-local message readable with fa_last_error().  Calls are re-entrant across streams.
 *
 * Reference interfaces replaced (paths relative to the reference repo):
 *   fa_tabulate_cells    ufcx `tabulate_tensor_float64` of the ffcx-compiled J form
 *                        (form built at FEniCSx/mechanic2d/asym_elasto_damage_model.cc:684-685
 *                        from FEniCSx/mechanic2d/asym_ufl.py:83) and MFEM
 *                        damIntegrator::AssembleElementGrad
 *                        (MFEM/mechanic2d/asym_elasto_damage_model.cc:639-916), batched over cells.
 *   fa_assemble_matrix   dolfinx::fem::assemble_matrix(set_block_fn(A, ADD_VALUES), J_form, {bcl,bcr})
 *                        + fem::set_diagonal(..., 1.0) as called from the setJ callback
 *                        (FEniCSx/mechanic2d/asym_elasto_damage_model.cc:847-862); MFEM
 *                        NonlinearForm::GetGradient driven from :1546.
 *   fa_build_adjacency,  dolfinx::fem::petsc::create_matrix(J_form) — the sparsity pattern of
 *   fa_sparsity_count,   (FEniCSx/mechanic2d/asym_elasto_damage_model.cc:688).
 *   fa_sparsity_fill
 *   fa_assemble_vector   dolfinx::fem::assemble_vector(b, F_form)
 *                        (FEniCSx/mechanic2d/asym_elasto_damage_model.cc:825) and MFEM
 *                        damIntegrator::AssembleElementVector (:559-637).
 *   fa_apply_lifting,    dolfinx::fem::apply_lifting / set_bc as called from setF
 *   fa_set_bc            (FEniCSx/mechanic2d/asym_elasto_damage_model.cc:827, :836).
 *   fa_facet_load_apply  the exterior_facet integrals of that assemble_vector: `- dot(t*n, delta_u)*ds(0)`
 *                        (FEniCSx/mechanic2d/asym_ufl.py:81; USE_SURF, asym_elasto_damage_model.cc:589-608).
 */
#ifndef FEMASM_H
#define FEMASM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FA_OK 0
#define FA_E_ARG (-1)       /* invalid argument (null pointer, bad size) */
#define FA_E_UNSUPPORTED (-2) /* element / form / quadrature combination not implemented */
#define FA_E_HIP (-3)       /* HIP runtime error (launch, allocation) */
#define FA_E_PATTERN (-4)   /* sparsity pattern missing an entry the mesh needs */
#define FA_E_CAPACITY (-5)  /* a row exceeds a kernel capacity (reported with sizes) */

/* dolfinx::mesh::CellType values */
#define FA_TRIANGLE 3
#define FA_QUADRILATERAL 4
#define FA_TETRAHEDRON (-4)
#define FA_HEXAHEDRON 8

/* Form kinds */
#define FA_LINEAR_ELASTICITY 0 /* sigma = lambda tr(eps) I + 2 mu eps  (reference J with d = 0) */
#define FA_ASYM_DAMAGE 1       /* reference mechanic2d damage law, P1 triangles (2-D plane strain) */
#define FA_NEO_HOOKEAN 2       /* compressible neo-Hookean, AD tangent */
#define FA_ASYM_DAMAGE_AD 3    /* FA_ASYM_DAMAGE with the tangent and stress of the reference's USE_AD build:
                                  forward-over-forward AD of its damage potential
                                  (MFEM/mechanic2d/asym_elasto_damage_model.cc:100-204, :752-763) */

/* fa_assemble_matrix flags */
#define FA_GATHER 0x0        /* row-gather: each BSR row computed once, plain coalesced stores */
#define FA_SCATTER 0x1       /* element-scatter with FP64 atomics (dolfinx/PETSc ADD_VALUES shape) */
#define FA_ZERO_FIRST 0x2    /* FA_SCATTER only: zero A->data first (MatZeroEntries) */
#define FA_DETERMINISTIC 0x4 /* FA_GATHER: bit-reproducible values, run to run (see below) */
#define FA_CHECK_ERRORS 0x8  /* validate the pattern and adjacency first (fa_check_pattern, when adj is given),
                                then synchronise `stream` and return FA_E_PATTERN if a kernel found a (row,
                                column) pair or a Dirichlet diagonal missing from the pattern (debugging) */
/* Deterministic assembly (FA_DETERMINISTIC, or FA_PLAN_DETERMINISTIC in plan->cell_flags, which
 * fa_gather_rows honours too): the row gather adds every element contribution v to a block as the
 * 64-bit integer round(v * 2^s_b) (s_b per BLOCK from a bound on the contributions of the cells adding
 * into it, |v 2^s_b| < 2^50) with integer LDS atomics, so each block's sum is exact and the same in any
 * order, then converts it back with one rounding: the values are identical run to run. Every cell
 * adding into block (a, b) holds node a, so a row's values are within ~2^-50 per summand of its own
 * cells' scale, at any stiffness contrast between rows (the per-row 1e-12 bar is tested at contrasts
 * 1e2 .. 1e8, tests/test_gpu_deterministic.py; rounds 4-5 had one scale per row chunk). For linear
 * elasticity with one Poisson ratio on affine simplices and (round 6) affine Q1 / Q2 quadrilaterals and Q1
 * hexahedra (the
 * k_gather_lin kernels) with a positional plan; other forms return FA_E_UNSUPPORTED. (The reference's MFEM integrator is likewise order-fixed: it runs
 * one thread, MFEM/mechanic2d/asym_elasto_damage_model.cc:27.) */

typedef struct {
  int32_t cell_type;     /* FA_TRIANGLE ... */
  int32_t degree;        /* Lagrange degree of the vector space (1, 2, 3) */
  int32_t gdim;          /* geometric dim = topological dim = block size bs (2 or 3) */
  int32_t nn;            /* nodes per cell of the space: dofmap width */
  int64_t ncells;
  int64_t nnodes;        /* number of space nodes (BSR block rows) */
  const int32_t* cells;  /* [ncells][nn] node dofmap, basix local ordering */
  int32_t nv;            /* geometry nodes per cell (P1 / Q1 vertices) */
  int32_t _pad;
  const int32_t* geom;   /* [ncells][nv] geometry dofmap */
  const double* x;       /* [nverts][gdim] vertex coordinates */
} fa_mesh;

typedef struct {
  int32_t kind;          /* FA_LINEAR_ELASTICITY ... */
  int32_t qdeg;          /* quadrature degree; < 0 = the degree UFL estimates for the form */
  const double* E;       /* [ncells] Young's modulus (DG0), or NULL to use lam/mu */
  double nu;             /* Poisson ratio (Constant) when E != NULL */
  const double* lam;     /* [ncells] Lame lambda when E == NULL */
  const double* mu;      /* [ncells] Lame mu when E == NULL */
  const double* u;       /* [nnodes*bs] state (damage, neo-Hookean, residual); may be NULL */
  const double* d;       /* [nnodes] damage (P1) for FA_ASYM_DAMAGE; may be NULL (= 0) */
  const double* f;       /* [nnodes*bs] body force (residual); may be NULL */
} fa_form;

typedef struct {
  int64_t nrows;         /* block rows = mesh nnodes */
  int32_t bs;            /* block size = gdim */
  int32_t _pad;
  int64_t nblocks;       /* indices length */
  const int64_t* indptr; /* [nrows+1] */
  const int32_t* indices;/* [nblocks], sorted per row */
  double* data;          /* blocks of rows [row_begin, row_end): [indptr[row_end]-indptr[row_begin]][bs][bs] */
  int64_t row_begin;     /* row window held by `data` (a row part of the matrix, or the rows a rank */
  int64_t row_end;       /* owns); row_end <= row_begin means the whole matrix [0, nrows) */
} fa_bsr;
/* A row window lets a caller hold the values of a row range only: a rank's owned rows, or a
 * matrix split into several allocations (femasm.la.MatrixCSR parts). */

typedef struct {
  const int64_t* ptr;    /* [nnodes+1] */
  const int32_t* idx;    /* [ncells*nn] flat dofmap positions p = cell*nn + local, sorted per node */
} fa_adjacency;

/* fa_plan.cell_flags */
#define FA_PLAN_AFFINE 0x1   /* every cell of a tensor mesh is a parallelogram / parallelepiped: its
                                hexahedra assemble through the affine row gather (no element-matrix
                                store); otherwise through the MFMA element kernel + block gather.
                                Every vertex within 1e-13 of the cell's size of the parallelepiped of
                                the edges at vertex 0 (the affine route's error is up to 3x that) */
#define FA_PLAN_DETERMINISTIC 0x2 /* set by the caller: assemblies with this plan (fa_assemble_matrix and
                                     fa_gather_rows) are deterministic, as with FA_DETERMINISTIC */
#define FA_PLAN_ORDER_SEARCH 0x4  /* set by the caller before fa_plan_order: search the LDS order harder (the
                                     chain search before the alignment and a second start from the
                                     equitable colouring, csrc/plan_order.h: config E 2 % fewer LDS passes,
                                     33.19 vs 33.15 ms per assembly (no gain), plan 1.1 -> 4.8 s) */
#define FA_PLAN_NEO 0x8           /* set by fa_plan_gather_form for FA_NEO_HOOKEAN: fa_plan_order orders
                                     the slots for the neo-Hookean kernel's item split */

/* Row-chunk plan for the gather kernel (host-computed once per pattern). */
typedef struct {
  int64_t nchunks;
  const int64_t* row_start;  /* device [nchunks+1] */
  int32_t max_blocks;        /* largest block count of a chunk */
  int32_t max_adj;           /* largest adjacency count of a chunk */
  const uint16_t* slots;     /* optional device [ncells*nn][nn]: for adjacency entry j and column
                                node b, the block's position within row j's column list */
  int32_t slot_order;        /* 0: `slots` is that plain map; > 0: fa_plan_order rewrote it for the
                                gather's item order (value = the kernel's column split) */
  int32_t cell_flags;        /* set by fa_plan_gather: FA_PLAN_AFFINE if every cell is affine */
  const int32_t* eadj;       /* positional plan (fa_plan_order with an entry buffer), else NULL:
                                each chunk's adjacency entries in the plan's bank-balanced order;
                                `slots` is then indexed by that position, chunk-relative */
  const int32_t* corder;     /* optional device [nchunks] (fa_plan_locality): the order in which the
                                gather visits its chunks; NULL = row order */
  const void* contrib;       /* optional contribution plan (fa_plan_contrib): P1/P2 simplices with
                                linear elasticity of one Poisson ratio then assemble through the
                                block-owner gather (no per-contribution LDS atomics) */
  const int64_t* chunk_desc; /* optional device [3 * (nchunks + 1)] (fa_plan_chunk_desc, round 6): the
                                store-decoupled gathers' per-chunk arrays in the visiting order, built
                                once per plan instead of at every launch; NULL = built per launch.
                                Rebuild (or set NULL) after changing corder or row_start */
} fa_plan;

const char* fa_last_error(void);
int fa_version(void);

/* Element metadata: nodes per cell and quadrature points for (cell_type, degree, qdeg). */
int fa_element_info(int32_t cell_type, int32_t degree, int32_t qdeg, int32_t* nn, int32_t* nq);

/* Host-only (no device call): whether an element's reference tensor Ahat (default rule for qdeg < 0)
 * is exactly N / D with small integers, i.e. packs into the integer table the store-decoupled gather
 * reads (simplices; affine quadrilaterals and Q1 hexahedra since round 6, e.g. Q2 quads: D = 180);
 * *packed_denom = D, or 0 when it does not pack (that element then assembles through the generic gather)
 * or for Q2 / Q3 hexahedra.
 * *amax = max |Ahat|. Either pointer may be NULL. */
int fa_element_table_info(int32_t cell_type, int32_t degree, int32_t qdeg, int32_t* packed_denom, double* amax);

/* Node -> cell adjacency (transpose of the dofmap): ptr [nnodes+1], idx [ncells*nn]. */
int fa_build_adjacency(const fa_mesh* mesh, int64_t* ptr, int32_t* idx, void* stream);

/* BSR sparsity: pass 1 writes indptr [nnodes+1] and returns the block count in *nblocks
 * (synchronises `stream` to read it); pass 2 fills indices [nblocks] sorted per row. */
int fa_sparsity_count(const fa_mesh* mesh, const fa_adjacency* adj, int64_t* indptr, int64_t* nblocks, void* stream);
int fa_sparsity_fill(const fa_mesh* mesh, const fa_adjacency* adj, const int64_t* indptr, int32_t* indices, void* stream);

/* Validate a sparsity pattern and its adjacency on the device (synchronises `stream`): indptr[0] = 0,
 * indptr monotone, indptr[nnodes] = nblocks; columns in [0, nnodes) and strictly increasing per row;
 * adjacency ptr[nnodes] = ncells*nn, entries of node r sorted, unique and at dofmap positions holding
 * r; every node of every cell present in the rows of the cell's nodes, and no other column (the
 * pattern dolfinx create_matrix builds). FA_E_PATTERN with the failed checks in fa_last_error().
 * The pattern and the adjacency come from rocPRIM sorts and scans (not code this library controls). */
int fa_check_pattern(const fa_mesh* mesh, const fa_adjacency* adj, const int64_t* indptr, const int32_t* indices,
                     int64_t nblocks, void* stream);

/* Gather plan: row chunks whose blocks and adjacency fit the kernel's LDS budget.
 * row_start is a caller-owned device buffer of capacity nnodes+1; nchunks etc. returned
 * in *plan (synchronises `stream`). */
int fa_plan_gather(const fa_mesh* mesh, const fa_adjacency* adj, const fa_bsr* A, int64_t* row_start, fa_plan* plan,
                   void* stream);

/* fa_plan_gather for the kernel of a form kind: FA_NEO_HOOKEAN chunks fill a larger accumulator
 * and aim at 128 adjacency entries (one round of the workgroup's 256 item lanes); other kinds are
 * fa_plan_gather. fa_assemble_matrix refuses a plan whose chunks exceed the form kernel's
 * accumulator (FA_E_ARG). Neo-Hookean forms assemble only with a positional plan (fa_plan_slots +
 * fa_plan_order with an entry buffer). */
int fa_plan_gather_form(const fa_mesh* mesh, int32_t kind, const fa_adjacency* adj, const fa_bsr* A,
                        int64_t* row_start, fa_plan* plan, void* stream);

/* Optional slot map for the gather plan (removes the per-block column search): slots is a
 * caller-owned device buffer of ncells*nn*nn uint16; on success plan->slots points to it.
 * Fails with FA_E_CAPACITY if a row holds more than 65535 blocks. */
int fa_plan_slots(const fa_mesh* mesh, const fa_adjacency* adj, const fa_bsr* A, uint16_t* slots, fa_plan* plan,
                  void* stream);

/* Bank-conflict-aware order for the gather's LDS adds (affine simplices, linear elasticity).
 * Each 16-lane quarter of a wave adds into LDS in passes set by its lanes' slots mod 16
 * (measured, tools/probe/lds_bank_probe.hip). With eadj == NULL, rewrites plan->slots in place so
 * that every lane of a quarter of the kernel's fixed item mapping visits its blocks in an order
 * that spreads each step over the banks; entries hold (b << 10) | position in the row. With eadj
 * (caller-owned device buffer of ncells*nn int32), the plan also chooses which adjacency entries
 * share a quarter (balancing their residues), writes each chunk's entries in that order to eadj,
 * and rewrites plan->slots by position with chunk-relative block positions (plan->eadj = eadj).
 * Sets plan->slot_order; a no-op (slot_order 0) for elements whose gather does not read an
 * ordered map. Run after fa_plan_slots for EVERY plan sharing the slot map (fa_plan_slots
 * rewrites all rows). */
int fa_plan_order(const fa_mesh* mesh, const fa_adjacency* adj, const fa_bsr* A, int32_t* eadj, fa_plan* plan,
                  void* stream);

/* Re-check plan->cell_flags & FA_PLAN_AFFINE against the mesh's CURRENT vertex coordinates (a
 * caller that moved vertices after fa_plan_gather): the affine tensor gather builds each cell's
 * Jacobian from three edge vectors, so a plan must not call a cell affine that no longer is.
 * Synchronises `stream`. A no-op for simplices (always affine). */
int fa_plan_check_affine(const fa_mesh* mesh, fa_plan* plan, void* stream);

/* Chunk visiting order for cache locality: chunks sorted by the Morton key of a point of each
 * chunk (the centroid of the cell of its first adjacency entry), so that chunks the gather runs
 * close in time share cells and their per-cell records stay in L2. corder is a caller-owned device
 * buffer of plan->nchunks int32; on success plan->corder points to it. Any permutation assembles
 * the same matrix (each chunk owns its rows); only the re-reads of the records change. */
int fa_plan_locality(const fa_mesh* mesh, const fa_adjacency* adj, int32_t* corder, fa_plan* plan, void* stream);

/* The chunk arrays the store-decoupled gathers (linear and neo-Hookean) read — per chunk, in the plan's
 * visiting order (plan->corder, or row order): its first block relative to A's row window, its first
 * adjacency entry, and its block and entry counts — into a caller-owned device buffer of
 * 3 * (plan->nchunks + 1) int64, once per plan (plan time, like the slot map); on success
 * plan->chunk_desc points to it and launches skip rebuilding them (config E: 0.21 ms per assembly, a
 * full read of the pattern's row pointer and adjacency pointer arrays). A must be the matrix (row
 * window) the plan was made for. Call it after fa_plan_locality. */
int fa_plan_chunk_desc(const fa_mesh* mesh, const fa_adjacency* adj, const fa_bsr* A, fa_plan* plan, int64_t* buf,
                       void* stream);

/* Block-owner gather (P1/P2 triangles and tetrahedra, linear elasticity with one Poisson ratio).
 * fa_plan_gather_contrib chunks the rows for it (like fa_plan_gather, smaller chunks: at most
 * 256 adjacency entries). fa_plan_contrib_bytes returns the device buffer size the contribution
 * plan of that chunking needs; fa_plan_contrib fills a caller-owned buffer of that size with
 * every chunk's (cell, row node, column node) contributions sorted by destination block and cut
 * into equal lane segments, and sets plan->contrib. The assembly then sums each block's
 * contributions in registers and writes it once (replaces the same dolfinx call as
 * fa_plan_gather: create_matrix + the cell loop of assemble_matrix,
 * FEniCSx/mechanic2d/asym_elasto_damage_model.cc:688, :852-857). */
int fa_plan_gather_contrib(const fa_mesh* mesh, const fa_adjacency* adj, const fa_bsr* A, int64_t* row_start,
                           fa_plan* plan, void* stream);
int fa_plan_contrib_bytes(const fa_mesh* mesh, const fa_adjacency* adj, const fa_bsr* A, const fa_plan* plan,
                          int64_t* bytes, void* stream);
int fa_plan_contrib(const fa_mesh* mesh, const fa_adjacency* adj, const fa_bsr* A, void* buf, int64_t bytes,
                    fa_plan* plan, void* stream);

/* Per-cell element matrices Ae [ncells_out][nn*bs][nn*bs] (dof = node*bs + comp) for cells
 * [c0, c0+ncells_out) — the batched ufcx tabulate_tensor / AssembleElementGrad. */
int fa_tabulate_cells(const fa_mesh* mesh, const fa_form* form, int64_t c0, int64_t ncells_out, double* Ae,
                      void* stream);

/* Global matrix assembly into A (BSR, pattern from fa_sparsity_*). bc: int8 per dof
 * (node*bs+comp) or NULL. Entries in bc rows/columns get no cell contribution and bc
 * diagonal entries are set to `diag` (dolfinx assemble_matrix + set_diagonal).
 * FA_GATHER needs adj and plan; FA_SCATTER needs neither (plan may be NULL). */
int fa_assemble_matrix(const fa_mesh* mesh, const fa_form* form, const fa_adjacency* adj, const fa_plan* plan,
                       const int8_t* bc, double diag, fa_bsr* A, int32_t flags, void* stream);

/* Split gather: fa_assemble_matrix(FA_GATHER) as two calls sharing a caller-owned work buffer
 * of fa_gather_work_bytes() bytes. fa_gather_prepare computes the per-cell records (geometry,
 * material, tangent, constrained-dof masks) for ALL cells; fa_gather_rows then assembles the
 * rows of `plan` (any sub-window of A: several plans over disjoint row ranges may be run in any
 * order, e.g. a rank's interface planes first, their exchange overlapping the interior rows).
 * `bc` must be the same in both calls. Same semantics per row as fa_assemble_matrix; elements /
 * forms without a gather kernel return FA_E_UNSUPPORTED. Neo-Hookean simplex forms prepare the
 * records of the M gather (k_gather_neo), whose plans must be positional (fa_plan_gather_form +
 * fa_plan_slots + fa_plan_order with an entry buffer); another plan is refused with FA_E_ARG
 * (by fa_assemble_matrix too). The library reads no environment variable: results and accepted
 * arguments depend on the arguments only.
 * (Replaces the same dolfinx call, FEniCSx/mechanic2d/asym_elasto_damage_model.cc:852-857, as
 * fa_assemble_matrix.) */
int fa_gather_work_bytes(const fa_mesh* mesh, const fa_form* form, int64_t* bytes);
int fa_gather_prepare(const fa_mesh* mesh, const fa_form* form, const int8_t* bc, void* work, void* stream);
int fa_gather_rows(const fa_mesh* mesh, const fa_form* form, const fa_adjacency* adj, const fa_plan* plan,
                   const int8_t* bc, double diag, const void* work, fa_bsr* A, void* stream);

/* Prepared cell state (fa_version() >= 105): fa_assemble_matrix(FA_GATHER) with the per-cell work that
 * stays the same across the assemblies of one mesh and one set of constrained dofs done once. A Newton
 * or load-stepping loop (the reference's setJ callback, FEniCSx/mechanic2d/asym_elasto_damage_model.cc:
 * 847-862, runs dolfinx assemble_matrix + set_diagonal at every iteration on one mesh with one bcs set)
 * changes only the coefficient E between assemblies. For FA_LINEAR_ELASTICITY with E per cell and one
 * Poisson ratio on the elements of the table gather (P2 / P3 triangles, P2 tetrahedra, affine Q1 / Q2
 * quadrilaterals, affine Q1 hexahedra) with a positional plan; every other form, element or plan:
 * FA_E_UNSUPPORTED from each call below, and the caller uses fa_assemble_matrix.
 *   static  rec [ncells][gdim^2 + 1, rounded up to even] doubles: sqrt(|det J| / D) J^-1 (D the packed
 *           reference table's denominator) and a word +1.0 holding the cell's constrained-dof bits in
 *           its low mantissa bits. Valid while the coordinates, the geometry dofmap, the dofmap and the
 *           bc marker are unchanged.
 *   static  diag_off [ndiag]: per (row window of A, bc marker), the offset in the window's `data` of
 *           every constrained dof's diagonal value (-1: skipped).
 *   per call  coef [ncells]: sign(mu_c) sqrt|mu_c|, rewritten by every assembly from form->E (8 B read
 *           and written per cell). Nothing keyed on the coefficient is kept.
 * The caller owns all three buffers. fa_prepared_bytes (host only) returns the sizes of rec and coef;
 * fa_prepare_diag_count the number of constrained dofs of A's row window (synchronises `stream`).
 * fa_prepare_cells fills rec (bc may be NULL: no bits; with bc the adjacency is required; `plan`, which
 * may be NULL for simplices, only says whether tensor cells are affine) and sets has_bc.
 * fa_prepare_diag fills `offsets` (capacity `count`) for A's row window and synchronises `stream`:
 * FA_E_PATTERN when a constrained dof has no diagonal block. fa_prepare_coef runs the coefficient pass
 * alone. fa_assemble_matrix_prepared = coefficient pass, the row gather of `plan` from rec and coef,
 * then `diag` stored at the listed offsets (nothing when has_bc is 0); the same values per row as
 * fa_assemble_matrix up to rounding (sqrt|mu| * sqrt|det J| against sqrt|mu det J|: ~1 ulp per
 * entry). It honours FA_DETERMINISTIC and FA_CHECK_ERRORS; FA_KEEP_COEF skips the coefficient pass
 * (the further row parts of one assembly, after the first part's call or fa_prepare_coef).
 * fa_gather_rows_prepared is fa_gather_rows on that state: the rows of `plan` (any sub-window of A,
 * with its own diagonal list in `prepared`), no coefficient pass (fa_prepare_coef once per assembly
 * takes the place of fa_gather_prepare). */
#define FA_KEEP_COEF 0x10 /* fa_assemble_matrix_prepared: coef is already this assembly's */
typedef struct {
  double* rec;             /* static records */
  double* coef;            /* per-call coefficients */
  const int64_t* diag_off; /* diagonal offsets of A's row window, or NULL */
  int64_t ndiag;
  int32_t has_bc;          /* set by fa_prepare_cells: the records hold constrained-dof bits */
  int32_t _pad;
} fa_prepared;
int fa_prepared_bytes(const fa_mesh* mesh, const fa_form* form, const fa_plan* plan, int64_t* rec_bytes,
                      int64_t* coef_bytes);
int fa_prepare_cells(const fa_mesh* mesh, const fa_form* form, const fa_adjacency* adj, const fa_plan* plan,
                     const int8_t* bc, fa_prepared* prepared, void* stream);
int fa_prepare_diag_count(const fa_mesh* mesh, const fa_bsr* A, const int8_t* bc, int64_t* count, void* stream);
int fa_prepare_diag(const fa_mesh* mesh, const fa_bsr* A, const int8_t* bc, int64_t* offsets, int64_t count,
                    void* stream);
int fa_prepare_coef(const fa_mesh* mesh, const fa_form* form, const fa_prepared* prepared, void* stream);
int fa_assemble_matrix_prepared(const fa_mesh* mesh, const fa_form* form, const fa_adjacency* adj, const fa_plan* plan,
                                const fa_prepared* prepared, double diag, fa_bsr* A, int32_t flags, void* stream);
int fa_gather_rows_prepared(const fa_mesh* mesh, const fa_form* form, const fa_adjacency* adj, const fa_plan* plan,
                            const fa_prepared* prepared, double diag, fa_bsr* A, void* stream);

/* Residual b += int sigma(u):eps(v) dx_q - int f.v dx_{2p} (b is ADDED into, like dolfinx
 * assemble_vector; the reference zeroes it first). sigma term on the form's quadrature degree
 * (the reference's `dxx`), load term on degree 2p (the reference's default `dx`). Node-parallel
 * through the adjacency: deterministic, one write per dof. u / f may be NULL (= 0). */
int fa_assemble_vector(const fa_mesh* mesh, const fa_form* form, const fa_adjacency* adj, double* b, void* stream);

/* dolfinx apply_lifting with one form: b[i] -= alpha * sum_j A_ij (g_j - x0_j) over bc
 * columns j, computed cell by cell with the cell matrices (bc rows i get no contribution;
 * set_bc overwrites them). The reference calls it with alpha = -1
 * (FEniCSx/mechanic2d/asym_elasto_damage_model.cc:827). g, x0 per dof (x0 may be NULL = 0). */
int fa_apply_lifting(const fa_mesh* mesh, const fa_form* form, const fa_adjacency* adj, double* b, const int8_t* bc,
                     const double* g, const double* x0, double alpha, void* stream);

/* b[i] = alpha * (g[i] - x0[i]) on bc dofs (x0 may be NULL). ndofs = nnodes*bs. */
int fa_set_bc(double* b, int64_t ndofs, const int8_t* bc, const double* g, const double* x0, double alpha,
              void* stream);

/* Per-cell expressions of the state: the reference's post-processing step, create_expression +
 * Function::interpolate into a DG0 space (FEniCSx/mechanic2d/asym_elasto_damage_model.cc:909-942, its
 * timing column 8.1) and MFEM's strainTensor / stressTensor coefficients projected on a DG space
 * (MFEM/mechanic2d/asym_elasto_damage_model.cc:332-457). Quantities (fa_version() >= 101): */
#define FA_EVAL_GRAD   0x1  /* grad u, row-major [gd][gd]: du_i/dx_j */
#define FA_EVAL_STRAIN 0x2  /* sym grad u, reduced: 2-D (xx, xy, yy); 3-D (xx, xy, xz, yy, yz, zz); tensor shear, not engineering */
#define FA_EVAL_STRESS 0x4  /* the form's law at w = 1: reduced Cauchy stress (same order) for FA_LINEAR_ELASTICITY,
                               FA_ASYM_DAMAGE, FA_ASYM_DAMAGE_AD; first Piola P row-major [gd][gd] for FA_NEO_HOOKEAN */
#define FA_EVAL_ENERGY 0x8  /* inner(eps, sigma), 1 value (small-strain laws; FA_NEO_HOOKEAN: FA_E_UNSUPPORTED) */
/* One launch evaluates every quantity whose output pointer is not NULL (grad u is shared) at the npts
 * reference points X of the cells cells[0 .. ncells_out) (ids in [0, mesh->ncells), not checked; NULL =
 * cells 0 .. ncells_out-1). Each output is [ncells_out][npts][value size], contiguous, 8-B aligned;
 * position k holds cell cells[k]. form->u is required (FA_E_ARG). Material per cell (E / nu or lam / mu);
 * the damage at a point is sum_a phi_a(X) d_a with the P1 basis (0 when form->d is NULL); the damage
 * kinds are P1-triangle only (FA_E_UNSUPPORTED otherwise). Every supported cell and degree, affine or
 * not: the Jacobian is taken at the point from the geometry basis. One lane per cell, no atomics:
 * deterministic. The tables at X are uploaded once per call (that upload waits for `stream`); for the
 * cell's single DG0 interpolation point (its midpoint) they are cached, and the call is asynchronous
 * and allocates nothing. Outputs of at most 16 doubles per cell and quantity, and 24 over all
 * quantities (every DG0 case) are stored coalesced, 16 B per lane; larger ones through plain per-lane
 * stores (the slow path). */
int fa_eval_cells(const fa_mesh* mesh, const fa_form* form,
                  int32_t npts, const double* X /* HOST [npts][tdim] reference points */,
                  const int32_t* cells /* device [ncells_out] cell ids, or NULL = cells 0..ncells_out-1 */,
                  int64_t ncells_out,
                  double* grad, double* strain, double* stress, double* energy, /* device; each may be NULL */
                  void* stream);

/* y = A x (block rows of A's window; x, y blocked dof vectors). The Krylov kernel of the Newton
 * driver that consumes the assembled matrix (the reference solves with CG + BoomerAMG,
 * FEniCSx/mechanic2d/asym_elasto_damage_model.cc:717-813). */
int fa_bsr_mult(const fa_bsr* A, const double* x, double* y, void* stream);

/* out[r - row_begin] = the diagonal block of block row r (zeros when absent), [rows, bs, bs]:
 * the block-Jacobi preconditioner of the driver's CG (the reference uses BoomerAMG, :717-813). */
int fa_bsr_block_diag(const fa_bsr* A, double* out, void* stream);

/* Matrix-free Jacobian action (fa_version() >= 102): the Krylov solve of the Newton driver with no
 * assembled matrix. The reference always assembles (MatSetValues into the PETSc matrix of
 * FEniCSx/mechanic2d/asym_elasto_damage_model.cc:688, solved at :717-813); these calls replace the pair
 * fa_assemble_matrix + fa_bsr_mult (and fa_bsr_block_diag) of that driver, not a reference interface.
 *
 * y = A x, where A is exactly the matrix fa_assemble_matrix(mesh, form, ..., bc, diag, ...) would hold,
 * evaluated at the form's current state form->u. Free row i: sum over free columns j of A_ij x_j (cell
 * contributions only). Constrained row i (bc[i] != 0): y_i = diag * x_i. Constrained columns contribute
 * nothing. y is overwritten (every dof written exactly once), not added into. x and y must not alias
 * (FA_E_ARG). `plan`: an apply plan (below) or NULL = the generic node-parallel kernel (every supported
 * cell, degree and form kind, affine or not). Deterministic: no atomics, bit-identical run to run. No
 * allocation, no synchronisation (the element tables are cached on the first call per element, as
 * everywhere). A plan must be the one built for this mesh and adjacency: the kernel checks its header
 * on the device and writes nothing when it does not match. */
int fa_apply_jacobian(const fa_mesh* mesh, const fa_form* form, const fa_adjacency* adj, const void* plan,
                      const int8_t* bc /* or NULL */, double diag, const double* x, double* y, void* stream);

/* out[a] = the diagonal block (a, a) of that same A, [nnodes][bs][bs] (zeroed bc rows / columns inside
 * the block, `diag` on constrained diagonal entries): the block-Jacobi preconditioner with no matrix.
 * Node-parallel through the adjacency, every supported element and form kind; bc may be NULL. */
int fa_jacobian_block_diag(const fa_mesh* mesh, const fa_form* form, const fa_adjacency* adj, const int8_t* bc,
                           double diag, double* out, void* stream);

/* Apply plan of the planned kernel (P1 / P2 triangles and tetrahedra, every form kind defined on them;
 * other elements: FA_E_UNSUPPORTED, use plan = NULL): a caller-owned, 8-byte aligned device buffer, built
 * once per (mesh, space), in the style of fa_plan_contrib_bytes / fa_plan_contrib. The rows are cut into
 * chunks of consecutive nodes whose distinct cells fit a 256-cell LDS tile; the buffer holds each chunk's
 * cell list and, per adjacency entry, the tile position of its (cell, local node) result: at most 6 bytes
 * per dofmap entry (ncells * nn) + 16 per chunk + 64. One workgroup per chunk then computes every
 * distinct cell's K_e(u) x_e once and sums the rows from the tile. Both calls synchronise `stream`
 * (_bytes to return the size; *nchunks may be NULL). A node with more cells than the tile holds:
 * FA_E_CAPACITY with the sizes in fa_last_error() (the caller then uses the generic kernel). Words 1 and 3
 * of the buffer's int64 header are the chunk count and the cell visits per launch (their ratio to ncells
 * is the redundancy left: 1 when no cell straddles chunks). */
int fa_apply_plan_bytes(const fa_mesh* mesh, const fa_adjacency* adj, int64_t* bytes, int64_t* nchunks, void* stream);
int fa_apply_plan(const fa_mesh* mesh, const fa_adjacency* adj, void* buf, int64_t bytes, void* stream);

/* ---- geometric multigrid: lattice transfers and the smoother step (femasm_mg.hip) ----
 * Not a reference interface: the reference preconditions its Krylov solve with BoomerAMG
 * (FEniCSx/mechanic2d/asym_elasto_damage_model.cc:720-813); these calls serve femasm.mg's geometric
 * multigrid on the structured meshes instead.
 *
 * A transfer joins a coarse lattice of nc[d] + 1 points per axis to the fine lattice of 2 nc[d] + 1
 * points (d < tdim; lattice index 0 fastest, the structured meshes' node numbering; dof = node * bs +
 * comp, bs 1 to 3). P is linear interpolation on the right-diagonal triangle / Kuhn tetrahedron mesh
 * (simplex = 1: a fine point I with odd mask o = I & 1 takes 1/2 of each of the coarse points
 * (I - o) / 2 and (I + o) / 2, or copies its coarse point when o = 0) or multilinear interpolation
 * (simplex = 0: the mean of the 2^|o| coarse points (I +- o) / 2). The same stencil is the P2 -> P1
 * transfer on one mesh and the P1(h) -> P1(2h) transfer between a mesh and its refinement. */
typedef struct {
  int32_t tdim;    /* 2 or 3 */
  int32_t simplex; /* 1: triangles / tetrahedra, 0: quadrilaterals / hexahedra */
  int32_t bs;      /* dofs per lattice point */
  int32_t _pad;
  int64_t nc[3];   /* coarse cells per axis (entries d >= tdim are ignored) */
} fa_transfer;

/* xf (+)= M_f P M_c xc: M zeroes the dofs whose marker is nonzero (bc_c / bc_f, int8 per dof, either
 * may be NULL). add = 0 overwrites xf (masked fine dofs receive 0), add != 0 adds into it (masked fine
 * dofs are left alone). One thread per fine dof gathers its coarse values: no atomics. */
int fa_prolong(const fa_transfer* t, const double* xc, const int8_t* bc_c /* or NULL */,
               const int8_t* bc_f /* or NULL */, int32_t add, double* xf, void* stream);

/* rc = M_c P^T M_f rf, the exact transpose of fa_prolong, as a gather per coarse dof: its own fine
 * point plus, for simplices, the fine points at +o and -o of every nonzero 0/1 vector o (weight 1/2; at
 * most 6 in 2-D, 14 in 3-D) or, for tensor cells, the 3^tdim - 1 neighbours (weight 2^-|o|); neighbours
 * outside the lattice are skipped. Fixed summation order, no atomics: bit-reproducible. rc is
 * overwritten. */
int fa_restrict(const fa_transfer* t, const double* rf, const int8_t* bc_f /* or NULL */,
                const int8_t* bc_c /* or NULL */, double* rc, void* stream);

/* One fused step of the Chebyshev / block-Jacobi smoother over nnodes * bs dofs (bs 1 to 3):
 *   d <- c_d d + c_r Dinv (b - Ax),   x <- x + d,
 * Dinv [nnodes][bs][bs] row-major. c_d == 0 does not read d (the first step of a polynomial); Ax may be
 * NULL for A x = 0 (a zero initial guess). One pass over the vectors. */
int fa_cheb_step(int64_t nnodes, int32_t bs, const double* Dinv, const double* b, const double* Ax /* or NULL */,
                 double c_d, double c_r, double* d, double* x, void* stream);

/* None of the three allocates or synchronises; all index arithmetic is 64-bit. */

/* ---- uniform refinement of simplex meshes and the transfers over the refined hierarchy
 * (femasm_refine.hip, fa_version() >= 104) ----
 * The reference scales its Gmsh mesh by uniform refinement (MAX_REFINE with refine, -r with
 * UniformRefinement); femasm.mesh.refine is regular ("red") refinement with a numbering chosen for the
 * multigrid: the parent's vertices keep their indices, the midpoint of edge e (edges in the
 * lexicographic order of their sorted vertex pair) is vertex nverts + e, the children of cell c are the
 * cells c * 2^tdim + k. That is the numbering of the parent's degree-2 nodes, so the P1 space on the
 * refined mesh has the nodes of the P2 space on the parent.
 *
 * fa_refine_cells: one thread per parent cell (FA_TRIANGLE: 4 children, FA_TETRAHEDRON: 8). cells
 * [ncells][nv] vertices, cell_edges [ncells][nl] edge ids in basix's local edge order, x [nverts][3]
 * vertex coordinates (tetrahedra only: the inner octahedron is split along the shortest of the diagonals
 * m01-m23, m02-m13, m03-m12, ties to the first; may be NULL for triangles), tags [ncells] or NULL.
 * Writes children [ncells * 2^tdim][nv] and, with tags, child_tags [ncells * 2^tdim]. Every child keeps
 * its parent's orientation sign. With m_ij the midpoint of local vertices i and j:
 *   triangle     (v0,m01,m02) (m01,v1,m12) (m02,m12,v2) (m01,m12,m02)
 *   tetrahedron  (v0,m01,m02,m03) (m01,v1,m12,m13) (m02,m12,v2,m23) (m03,m13,m23,v3), then around
 *     m01-m23:   (m01,m02,m03,m23) (m01,m03,m13,m23) (m01,m12,m23,m13) (m01,m02,m23,m12)
 *     m02-m13:   (m01,m02,m03,m13) (m01,m02,m13,m12) (m02,m03,m13,m23) (m02,m12,m23,m13)
 *     m03-m12:   (m01,m02,m03,m12) (m02,m03,m12,m23) (m03,m12,m23,m13) (m01,m03,m13,m12) */
int fa_refine_cells(int32_t cell_type, int64_t ncells, int64_t nverts, const int32_t* cells,
                    const int32_t* cell_edges, const double* x /* or NULL */, const int32_t* tags /* or NULL */,
                    int32_t* children, int32_t* child_tags /* or NULL */, void* stream);

/* xm[e][d] = 0.5 * (x[a][d] + x[b][d]) for edge e = (a, b) of edge_verts [nedges][2]; x [.][gdim], xm
 * [nedges][gdim]. One thread per edge and component. */
int fa_edge_midpoints(int64_t nedges, int32_t gdim, const int32_t* edge_verts, const double* x, double* xm,
                      void* stream);

/* Transfer between ncoarse coarse nodes and ncoarse + nedges fine nodes (dof = node * bs + comp): P is
 * the identity on the first ncoarse fine nodes and 1/2, 1/2 on an edge node. */
typedef struct {
  int64_t ncoarse;            /* coarse nodes; fine nodes = ncoarse + nedges, fine node ncoarse + e is edge e */
  int64_t nedges;
  int32_t bs, _pad;           /* dofs per node, 1..3 */
  const int32_t* edge_verts;  /* [nedges][2] coarse nodes of each edge */
  const int64_t* vptr;        /* [ncoarse + 1] CSR: the edges of each coarse node ... */
  const int32_t* vedges;      /* [2 nedges]    ... in ascending edge order */
} fa_edge_transfer;

/* xf (+)= M_f P M_c xc and rc = M_c P^T M_f rf with the marker and add rules of fa_prolong /
 * fa_restrict. Both gather (one thread per output dof; the restriction sums a node's own fine dof, then
 * its edges in vedges order, whatever the node's valence): no atomics, no allocation, no
 * synchronisation, 64-bit index arithmetic, bit-reproducible. */
int fa_prolong_edges(const fa_edge_transfer* t, const double* xc, const int8_t* bc_c /* or NULL */,
                     const int8_t* bc_f /* or NULL */, int32_t add, double* xf, void* stream);
int fa_restrict_edges(const fa_edge_transfer* t, const double* rf, const int8_t* bc_f /* or NULL */,
                      const int8_t* bc_c /* or NULL */, double* rc, void* stream);

/* ---- exterior-facet loads: surface tractions and pressure (femasm_facet.hip, fa_version() >= 106) ----
 * The facet term of the reference's residual, `- dot(t*n, delta_u)*ds(0)` (FEniCSx/mechanic2d/asym_ufl.py:81,
 * with the exterior_facet subdomain data of its "5.2 Neumann setting", asym_elasto_damage_model.cc:589-608,
 * switched off there for a dolfinx 0.8.0 bug in pack_coefficient_entity): what dolfinx::fem::assemble_vector
 * adds for the exterior_facet integrals of a linear form.
 *
 *   b[a, i] += alpha * sum over the loaded facets F of node a of  int_F (t_i - p n_i) phi_a dS
 *
 * on the REFERENCE configuration (dead loads: nothing depends on the state u, so there is no tangent).
 * t is a force per reference area, p a pressure along the reference OUTWARD unit normal n: the traction of
 * a pressure is -p n (the reference's scalar t in t*n is -p). At a facet point X (cell reference
 * coordinates) J = sum_v x_v (x) grad psi_v(X) with the P1 / Q1 geometry basis and, by Nanson's formula,
 *   n dS = sign(det J) cof(J) N_ref dS_ref     (cof(J) = det(J) J^-T, formed without the inverse),
 * outward for either cell orientation; dS = |n dS|. J is taken at every point: bilinear hexahedron faces
 * and non-affine quadrilaterals are integrated as they are. Facet rule: Gauss on [0, 1] (2-D), the
 * library's triangle / quadrilateral rule (3-D) of degree qdeg, mapped into the cell through the local
 * facet's reference vertices X = V0 + xi (V1 - V0) + eta (V2 - V0).
 *
 * The plan (host-built once per facet set, all DEVICE arrays): the loaded facets as slots 0 .. nfacets-1
 * (femasm sorts them by facet id), each with its one cell and its local facet index in basix's
 * sub-entity numbering (triangle edges (1,2),(0,2),(0,1); quadrilateral edges (0,1),(0,2),(1,3),(2,3);
 * tetrahedron face i opposite vertex i; hexahedron faces (0,1,2,3),(0,1,4,5),(0,2,4,6),(1,3,5,7),
 * (2,3,6,7),(4,5,6,7)); the loaded nodes as a compact list with a CSR over entries slot * nk + k, where
 * k counts the nodes of the local facet's closure in ascending local node order (nk per facet: p + 1 on
 * an edge, (p+1)(p+2)/2 on a triangle, (p+1)^2 on a quadrilateral face). A node's entries are summed in
 * the order stored (femasm: ascending slot), one thread per loaded node, one write per dof, no atomics:
 * bit-identical run to run. Entries, cells, local facets, value rows and nodes out of range are skipped
 * on the device, never dereferenced. */
#define FA_LOAD_NONE 0     /* the value is absent (its pointer is ignored) */
#define FA_LOAD_CONSTANT 1 /* one value for every facet: traction [gdim], pressure [1] */
#define FA_LOAD_FACET 2    /* one value per facet: traction [nvalues][gdim], pressure [nvalues]; slot s reads row
                              facet_value[s] */
#define FA_LOAD_NODAL 3    /* nodal values in the mesh's space, interpolated with the cell basis at the facet
                              points: traction [nnodes][gdim], pressure [nnodes] */
typedef struct {
  int64_t nfacets;             /* loaded facets (slots) */
  int64_t nloaded;             /* loaded nodes */
  int64_t nvalues;             /* rows of the FA_LOAD_FACET value arrays */
  int32_t nk;                  /* nodes in a facet's closure (checked against the element) */
  int32_t qdeg;                /* facet quadrature degree; < 0 = 2 * degree (the rule of the f.v dx term) */
  const int32_t* facet_cell;   /* [nfacets] the facet's cell */
  const int32_t* facet_local;  /* [nfacets] its local facet index in that cell */
  const int32_t* facet_value;  /* [nfacets] its row of the per-facet value arrays */
  const int32_t* nodes;        /* [nloaded] loaded nodes, each once */
  const int64_t* node_ptr;     /* [nloaded + 1] CSR over entries */
  const int32_t* entries;      /* [node_ptr[nloaded]] slot * nk + k */
  int32_t traction_mode;       /* FA_LOAD_* */
  int32_t pressure_mode;       /* FA_LOAD_* */
  const double* traction;      /* DEVICE values, read at every call */
  const double* pressure;
} fa_facet_load;

/* b += alpha * (the integral above). Asynchronous; no allocation and no synchronisation after the first
 * call per (element, qdeg), which caches the facet tables on the device like the cell tables. Every
 * supported cell type and degree (P1 / P2 simplices, Q1 .. Q3). Replaces the exterior_facet part of
 * dolfinx::fem::assemble_vector(b, L) for L = dot(t, v)*ds(k) - p*dot(n, v)*ds(k). Out of scope: follower
 * (deformation-dependent) pressure and its unsymmetric tangent, interior-facet and Robin terms. */
int fa_facet_load_apply(const fa_mesh* mesh, const fa_facet_load* load, double alpha, double* b, void* stream);

/* ---- scalar functionals: energy and norm integrals (femasm_scalar.hip, fa_version() >= 107) ----
 * dolfinx.fem.assemble_scalar for the integrands the library's forms define. The reference validates
 * itself by displacement and energy errors; its energy is the integral of the potential whose derivative
 * is the residual F_form (FEniCSx/mechanic2d/asym_ufl.py:78-81).
 *
 * fa_quadrature: the library's rule of degree qdeg (0 .. 12; 0 is the degree-1 rule) on the reference
 * cell, HOST arrays, no device call: pts [nq][tdim], wts [nq]. With pts and wts both NULL only *nq is
 * written; otherwise *nq holds the capacity of the arrays on entry (FA_E_ARG when short) and the point
 * count on return. The rule every kernel here integrates with (make_quadrature). */
int fa_quadrature(int32_t cell_type, int32_t qdeg, int32_t* nq, double* pts /* HOST */, double* wts /* HOST */);

#define FA_FUNC_MEASURE 0       /* int 1 dx; rule qdeg, default max(1, the form estimate): exact on affine cells */
#define FA_FUNC_STRAIN_ENERGY 1 /* int psi(grad u) dx of form's law on the rule of fa_assemble_vector's sigma term
                                   (qdeg < 0: form->qdeg, and if that is < 0 the estimate; the damage kinds: always
                                   their single point). FA_LINEAR_ELASTICITY: lam/2 tr(eps)^2 + mu eps:eps;
                                   FA_NEO_HOOKEAN: mu/2 (I_C - 3) - mu ln J + lam/2 (ln J)^2 at F = I + grad u (a cell
                                   with J <= 0 yields NaN or inf, which reaches the total); FA_ASYM_DAMAGE(_AD): the
                                   reference's damage potential (MFEM/mechanic2d/asym_elasto_damage_model.cc:100-155)
                                   with d the mean of the cell's three nodal values, the linear potential for d <= 0 */
#define FA_FUNC_L2 2            /* int sum_i (w_i - g_i)^2 dx; rule qdeg, default 2 * degree */
#define FA_FUNC_H1 3            /* int sum_ik (d_k w_i - G_ik)^2 dx; rule qdeg, default 2 * degree */
/* fa_assemble_scalar: cell_out[c] = the integral over cell c (every cell visited once, one lane per cell,
 * plain stores; NULL = kept in the workspace) and *total = their sum (NULL = no sum): per 256-cell tile a
 * binary tree over the tile's entries, then the tile partials by one workgroup in a fixed order. No
 * floating-point atomics: the total is bit-identical run to run and does not depend on the launch grid.
 * w: the nodal field [nnodes][gdim] of FA_FUNC_L2 / FA_FUNC_H1 (ignored otherwise; the energies read
 * form->u, which is required). g: FA_FUNC_L2 values [ncells][nq][gdim], FA_FUNC_H1 values
 * [ncells][nq][gdim][gdim] at the rule's points, or NULL for zero. form may be NULL except for
 * FA_FUNC_STRAIN_ENERGY. work: caller-owned, 8-byte aligned, at least fa_functional_work_bytes() bytes
 * (host only); required when total is given. Asynchronous on `stream`; no allocation after the first call
 * per (element, rule), which caches the tables. ncells == 0 writes +0.0 to *total with no cell launch.
 * Null or short arguments: FA_E_ARG. Every supported element (P1 / P2 simplices, Q1 .. Q3); the damage
 * kinds on P1 triangles only (FA_E_UNSUPPORTED otherwise). */
int fa_functional_work_bytes(const fa_mesh* mesh, int64_t* bytes);
int fa_assemble_scalar(const fa_mesh* mesh, const fa_form* form, int32_t kind, const double* w, const double* g,
                       int32_t qdeg, double* cell_out /* [ncells] or NULL */, void* work, int64_t work_bytes,
                       double* total /* device double or NULL */, void* stream);

/* ---- point location and evaluation at arbitrary points (femasm_points.hip, fa_version() >= 108) ----
 * dolfinx.geometry.bb_tree + compute_collisions_points + compute_colliding_cells, and Function.eval: which cell
 * holds a physical point, where in the cell, and a finite-element field's value and gradient there. The
 * reference compares displacements computed on different meshes by matching dof coordinates (the IN_COMP block
 * of FEniCSx/mechanic2d/asym_elasto_damage_model.cc sorts them and throws when a node has no twin; doc.tex,
 * figure ref2_mesh_difference); with these two calls the meshes need not share nodes or cells.
 *
 * The plan (host-built once per mesh and coordinates, all DEVICE arrays; femasm.geometry.bb_tree): a uniform
 * grid over the box of the cells' PADDED bounding boxes. A cell is listed in every bin its padded box meets;
 * the padding must cover the tolerance, i.e. every point a cell accepts lies in that cell's padded box
 * (femasm pads by 1e-6 of the box diagonal and requires tol <= a quarter of that factor). */
typedef struct {            /* uniform grid over the mesh's (padded) bounding box */
  int32_t dims[3];          /* bins per axis (entries d >= gdim are 1) */
  int32_t _pad;
  double lo[3], inv_h[3];   /* bin of x along d: clamp(floor((x[d]-lo[d])*inv_h[d]), 0, dims[d]-1) */
  const int64_t* bin_ptr;   /* [nbins+1], bin index = (k*dims[1]+j)*dims[0]+i */
  const int32_t* bin_cells; /* cells whose padded bounding box meets the bin, ASCENDING cell id per bin */
} fa_cell_grid;

/* cell[i] = the SMALLEST id among the cells that accept point x[i] (unique on shared vertices, edges and
 * faces, whatever the grid), X[i] = the point's reference coordinates in that cell; no cell accepts:
 * cell[i] = -1 and X[i] = NaN. One lane per point: with t_d = (x[d] - lo[d]) * inv_h[d], a point with some
 * t_d outside [0, dims[d]] (outside the grid's box; a NaN or infinite coordinate) is rejected without reading
 * a bin; otherwise the lane walks its bin's cells in stored order and stops at the first that accepts.
 *
 * Acceptance rule (the definition; femasm.geometry's host path applies the same one). Vertex 0 is subtracted
 * first: e_v = x_v - x_v0, dx = x - x_v0.
 *   triangles, tetrahedra   J = [e_1 .. e_tdim]; X = adj(J) dx / det J (cofactor form, either sign of det J:
 *       mirrored cells are cells); lambda_0 = 1 - sum X, lambda_k = X_(k-1); accept when every lambda_i >= -tol.
 *   quadrilaterals, hexahedra   Newton on the Q1 map from the centre X = 1/2: r = sum_v psi_v(X) e_v - dx,
 *       J = sum_v e_v (x) grad psi_v(X), X <- X - adj(J) r / det J; at most 12 steps; converged when a step has
 *       |dX|_inf <= 1e-12 (an affine cell: the first step lands, the second confirms). A step whose det J has
 *       not the sign of det J at the centre, or that leaves [-1, 2]^tdim, rejects the CELL (the walk goes on),
 *       as does running out of steps. Accept when converged and -tol <= X_d <= 1 + tol for every d.
 * tol is in reference coordinates (femasm: 1e-10). mesh->geom / x are read (mesh->cells only for the
 * argument check). Entries of bin_cells outside [0, ncells) are skipped, never dereferenced.
 * Asynchronous, no allocation, no atomics, 64-bit index arithmetic; npts == 0 launches nothing. Null or
 * short arguments, a grid with a dimension < 1 or tol < 0: FA_E_ARG; an unsupported element: FA_E_UNSUPPORTED. */
int fa_locate_points(const fa_mesh* mesh, const fa_cell_grid* grid, int64_t npts, const double* x /*[npts][gdim]*/,
                     double tol, int32_t* cell /*[npts]*/, double* X /*[npts][gdim]*/, void* stream);

/* val[i][r] = sum_a phi_a(X_i) w[node_a][r] and grad[i][r][j] = sum_a w[node_a][r] (grad_X phi_a(X_i) . J(X_i)^-1)_j
 * in cell cell[i], with the space's Lagrange basis evaluated on the device at each point's own X (P1 / P2
 * simplices: closed form in the barycentrics, basix node order; Q1 .. Q3: products of 1-D Lagrange polynomials
 * on the element's own nodes, equispaced for p <= 2 and GLL for p = 3, the node positions and the node <->
 * lattice map uploaded once per element from the host definition) and J from the P1 / Q1 geometry at X,
 * inverted in cofactor form. mesh->cells / degree / nn are the space's dofmap; w [nnodes][bs], bs 1 .. 3 (any
 * block size, not only gdim). Rows with cell[i] < 0 (or >= ncells) get NaN and read nothing. Either output
 * may be NULL, not both. One lane per point, no atomics: deterministic. Asynchronous; no allocation after the
 * first call per tensor element, which caches that table. Every element fa_eval_cells takes, affine or not.
 * npts == 0 launches nothing. Null arguments, bs outside 1 .. 3: FA_E_ARG; unsupported element: FA_E_UNSUPPORTED. */
int fa_eval_points(const fa_mesh* mesh /* its cells/degree/nn are the space's dofmap */, const double* w /*[nnodes][bs]*/,
                   int32_t bs /*1..3*/, int64_t npts, const int32_t* cell, const double* X,
                   double* val /*[npts][bs] or NULL*/, double* grad /*[npts][bs][gdim] or NULL*/, void* stream);

/* ---- smoothed-aggregation algebraic multigrid (femasm_amg.hip, fa_version() >= 109) ----
 * The reference preconditions with BoomerAMG on a mesh nobody refined; femasm.mg.SmoothedAggregation builds
 * its coarse levels from the matrix and the node coordinates alone (rigid-body modes as the near-null
 * space). Aggregates, sparsity patterns and product lists are set-up work of the caller (femasm: torch
 * ops on the device, once); these calls are what runs at every Newton step and inside the V-cycle. None
 * of them allocates or synchronises, all index arithmetic is 64-bit, all sums run in a fixed order with
 * no atomics (bit-identical run to run), and an index outside its operand is skipped, never dereferenced.
 *
 * fa_bcsr_mult: y (+)= B x for a block-CSR matrix of nrows x ncols blocks, each [br][bc] row-major:
 * indptr [nrows + 1], indices [nblocks] block columns, data [nblocks][br][bc]; x [ncols * bc], y
 * [nrows * br]; add = 0 overwrites y. Block shapes (2,3), (3,2), (3,3), (3,6), (6,3), (6,6): a
 * prolongator, its stored transpose (the restriction as a gather: the exact transpose) and the coarse
 * matrices with 6-dof nodes; anything else is FA_E_UNSUPPORTED. Eight lanes share a block row. */
int fa_bcsr_mult(int64_t nrows, int64_t ncols, int32_t br, int32_t bc, const int64_t* indptr, const int32_t* indices,
                 const double* data, const double* x, int32_t add, double* y, void* stream);

/* fa_bcsr_product: the numeric phase of a block SpGEMM on a precomputed inverted list,
 *   out[s] = sum over q in [optr[s], optr[s + 1]) of X[xa[q]] * Y[yb[q]],   s < nout,
 * X blocks [r][k], Y blocks [k][c], out blocks [r][c], all row-major; xa / yb are block slots of X (< nx)
 * and Y (< ny), nprod the length of the lists. An empty range gives a zero block. Shapes (r, k, c):
 * (2,2,3), (3,3,3), (3,3,6), (6,6,6) (A*T, A*P) and (3,2,3), (6,3,6) (P^T*Y); anything else is
 * FA_E_UNSUPPORTED. A group of lanes per output block, lane = (row of the block, stride offset into the
 * list): a wave when nprod > 8 nout, a quarter wave otherwise; partial sums meet in a fixed tree. */
int fa_bcsr_product(int64_t nout, int32_t r, int32_t k, int32_t c, const int64_t* optr, int64_t nprod,
                    const int32_t* xa, const int32_t* yb, const double* X, int64_t nx, const double* Y, int64_t ny,
                    double* out, void* stream);

/* The contract of fa_cheb_step at bs = 6 (fa_cheb_step itself serves bs 1 to 3). */
int fa_cheb_step6(int64_t nnodes, const double* Dinv, const double* b, const double* Ax /* or NULL */, double c_d,
                  double c_r, double* d, double* x, void* stream);

/* out[i] = free_nodes[i] ? max over k in row i of in[indices[k]] : 0 (free_nodes NULL: every row is free; an
 * empty row gives 0); in [nin], out [nrows], int64. The graph primitive of the deterministic MIS(2)
 * aggregation; the few rounds are driven by the caller. */
int fa_csr_row_max(int64_t nrows, const int64_t* indptr, const int32_t* indices, const int8_t* free_nodes /* or NULL */,
                   const int64_t* in, int64_t nin, int64_t* out, void* stream);

/* ---- vertex graph: the damage field's spread (femasm_graph.hip, fa_version() >= 110) ----
 * The reference builds its damage field d from tagged edges before it assembles the damage law: the tagged
 * entities' vertices are set to d_max and the marks are spread over the vertex graph (FEniCSx/mechanic2d/
 * asym_elasto_damage_model.cc:315-475, MFEM/mechanic2d/asym_elasto_damage_model.cc:1159-1315). On one
 * process, without its ownership bookkeeping, that is the definition below.
 *
 * G is the vertex graph as CSR: indptr [nverts + 1], indices [indptr[nverts]] (int32), row v the neighbours
 * N(v) of vertex v in ascending index, no self loops, no duplicates; inv_deg[v] = 1 / |N(v)|, and 0 where
 * N(v) is empty (such a vertex keeps its value). One iteration is two Jacobi passes, each reading only the
 * previous field and writing a new one:
 *   gated   s(v) = sum over w in N(v) of d(w) if d(v) < threshold, else 0;   d'(v)  = max(s(v) * inv_deg[v], d(v))
 *   full    s(v) = sum over w in N(v) of d'(w);                              d''(v) = max(s(v) * inv_deg[v], d'(v))
 * The arithmetic is part of the definition: s starts at 0.0 and adds the row in its stored order, the sum
 * is multiplied by the stored reciprocal (not divided by the degree), then the maximum is taken; no product
 * is followed by an add, so no FMA forms, and a sequential loop over the same arrays gives the same bits.
 *
 * d [nverts] holds the start field (finite, >= 0) and receives the result; tmp [nverts] is scratch. One lane
 * per vertex, 2 * iterations launches on `stream` that alternate d -> tmp (gated) and tmp -> d (full).
 * Asynchronous, no allocation, no atomics, no LDS, 64-bit index arithmetic; an index outside [0, nverts) is
 * skipped, never dereferenced. threshold may be +inf (every vertex takes the gated pass) or 0 (none does).
 * nverts == 0 or iterations == 0 launches nothing and succeeds. Checked on the host before anything is
 * launched: nverts < 0, iterations < 0 or a null pointer: FA_E_ARG; nverts > INT32_MAX: FA_E_CAPACITY. */
int fa_vertex_spread(int64_t nverts, const int64_t* indptr, const int32_t* indices, const double* inv_deg,
                     double* d /* in: start field; out: result */, double* tmp /* [nverts] scratch */,
                     int32_t iterations, double threshold, void* stream);

/* Measurement helper (not part of the reference interface): a 16-B-per-lane grid-stride stream
 * over n doubles (n even, 16-B aligned buffers) for the measured HBM peak beside the 8 TB/s spec
 * (SURVEY.md section 8(d)). mode 0: dst = src (copy), 1: dst = 1.0 (write only), 2: read src
 * (dst receives one partial sum per workgroup; n >= 8 * CUs). Asynchronous on `stream`. */
int fa_hbm_probe(int32_t mode, double* dst, const double* src, int64_t n, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FEMASM_H */
