"""Seeded, developed states for the spectral RK kernels, and the oracles that judge runs from them (no GPU).

From rest the flow sits in the rows under the lid for the first iterations: v is tiny and, away from the lid, every quadratic
term of the residual is far below the 1e-12 state tolerance of the suite -- a kernel that drops the convective terms on half
the cavity passes every from-rest test (test_spectral_seeded_cpu.py pins that).  ``seed_state`` puts an O(1) field on every
node instead, one node off every wall included, so that every tile of every mapping carries signal from the first residual.

``MutantSG`` is the oracle with one arithmetic fault (what a subtly wrong kernel would compute), ``ReorderedSG`` the oracle
with every contraction summed in reversed index order (what another correct kernel would compute: the rounding floor).
``CASES`` is the matrix that tests/test_gpu_spectral_seeded.py runs on the device and tests/test_spectral_seeded_cpu.py
qualifies here: the floor must stay a hundred times below the GPU tolerances, every fault a hundred times above them.
"""
from __future__ import annotations

from dataclasses import dataclass, field, replace

import numpy as np

from oracle import ldc_oracle as orc
from test_gpu_xcd import oracle_rows          # noqa: F401  (the K x 8 record table; it takes any oracle, seeded ones too)

KINDS = ("noconv_lower", "vuy_tile", "swap_vx_tile", "lapv_y_tile", "px_ring", "last_tile")


def seed_state(o, seed, amp=0.3, bc=True):
    """u, v (full grid) and p (inner grid) of ``o`` set to amp * (nine sine modes with normal coefficients), boundary values
    imposed (``bc=False``: left as the sines give them, nonzero on all four edges).  Returns copies for ``SGSolver.set_state``.
    No envelope: the field is O(1) one node off every wall, so corner and edge tiles carry signal too."""
    X, Y = np.meshgrid(o.ax.x, o.ay.x, indexing="ij")
    rng = np.random.default_rng(seed)

    def f():
        return sum(rng.standard_normal() * np.sin((a + 1) * X + b * Y) for a in range(3) for b in range(3))

    u, v, p = amp * f(), amp * f(), np.ascontiguousarray(amp * f()[1:-1, 1:-1])
    if bc:
        o.apply_bc(u, v)
    o.u, o.v, o.p = u, v, p
    return u.copy(), v.copy(), p.copy()


def _tile_of(index):
    i0 = 16 * (index // 16)
    return slice(i0, i0 + 16)


def _residual(o, u, v, p, mm, kind=None):
    """OracleSG.residual term by term (bit for bit with ``mm = np.matmul`` and no ``kind``), with room for one fault."""
    Dx, Dy, D2x, D2y = o.ax.D, o.ay.D, o.ax.D2, o.ay.D2
    ux, uy = mm(Dx, u), mm(u, Dy.T)
    vx, vy = mm(Dx, v), mm(v, Dy.T)
    lap_u = mm(D2x, u) + mm(u, D2y.T)
    lvx, lvy = mm(D2x, v), mm(v, D2y.T)
    pf = mm(mm(o.ax.I, p if o.stage_pressure else o.p), o.ay.I.T)
    px, py = mm(Dx, pf), mm(pf, Dy.T)
    uux, vuy, uvx, vvy = u * ux, v * uy, u * vx, v * vy
    cx, cy = _tile_of(o.M // 2), _tile_of(o.My // 2)             # the 16 x 16 tile that holds the centre node
    if kind == "noconv_lower":
        for t in (uux, vuy, uvx, vvy):
            t[:, : o.My // 2] = 0.0
    elif kind == "vuy_tile":
        vuy[cx, cy] = 0.0
    elif kind == "swap_vx_tile":
        uvx[:16, :16] = (u * vy)[:16, :16]
    elif kind == "lapv_y_tile":
        lvy[cx, cy] = 0.0
    elif kind == "px_ring":
        px[1, :] = 0.0
    elif kind == "last_tile":
        uux[_tile_of(o.M - 2), _tile_of(o.My - 2)] = 0.0
    elif kind is not None:
        raise ValueError(f"unknown fault: {kind}")
    nu = 1.0 / o.Re
    Ru = -(uux + vuy) - px + nu * lap_u
    Rv = -(uvx + vvy) - py + nu * (lvx + lvy)
    Rp = -o.beta2 * (ux + vy)[1:-1, 1:-1]
    return Ru, Rv, Rp


class MutantSG(orc.OracleSG):
    """The oracle with ONE arithmetic fault in its residual (``kind``, one of KINDS; None: no fault):
    noconv_lower -- convection dropped for j < My // 2;  vuy_tile -- v u_y dropped in the centre 16 x 16 tile;
    swap_vx_tile -- v_x replaced by v_y in rows and columns 0 ... 15;  lapv_y_tile -- v D2y^T dropped in the centre tile;
    px_ring -- dp/dx dropped on row i = 1;  last_tile -- u u_x dropped in the 16 x 16 block that holds index M - 2."""
    kind = None

    def residual(self, u, v, p, want_parts=False):
        return _residual(self, u, v, p, np.matmul, self.kind)


def _reversed_matmul(A, B):
    return np.matmul(np.ascontiguousarray(A[:, ::-1]), np.ascontiguousarray(B[::-1, :]))


class ReorderedSG(orc.OracleSG):
    """The same residual with every contraction summed in reversed index order."""

    def residual(self, u, v, p, want_parts=False):
        return _residual(self, u, v, p, _reversed_matmul)


# --------------------------------------------------------------------------------------------------- the case matrix
PARAMS = dict(Lx=2.0, Ly=1.0, lid_velocity=1.5, CFL=0.8, beta_squared=2.0)
SAAD = dict(PARAMS, corner_treatment="saad")


@dataclass(frozen=True)
class Case:
    """One seeded run.  ``mode``: the kernel that must advance it (0 launch path, 3 one XCD, 4 one CU, 5 chip-wide);
    ``persistent``: what the solver is asked for where that differs; ``layout``: LDC_WIDE_LAYOUT (None: the library's choice);
    ``kw``: oracle / solver parameters away from their defaults; ``bc=False``: the seed keeps nonzero edges."""
    id: str
    mode: int
    N: int
    ny: int = None
    Re: float = 400.0
    K: int = 4
    amp: float = 0.3
    seed: int = 0
    smoother: bool = False
    diagnostics: bool = True
    layout: str = None
    kw: dict = field(default_factory=dict)
    bc: bool = True
    persistent: int = None

    def oracle(self, cls=orc.OracleSG):
        o = cls(self.N, self.Re, ny=self.ny, stage_pressure=self.smoother, **self.kw)
        return o, seed_state(o, self.seed, self.amp, self.bc)

    def solver_kw(self):
        d = dict(name="spectral", Re=float(self.Re), lid_velocity=1.0, Lx=1.0, Ly=1.0, nx=self.N,
                 ny=self.N if self.ny is None else self.ny, tolerance=1e-6, max_iterations=10_000_000,
                 basis_type="chebyshev", CFL=1.5, beta_squared=5.0, corner_treatment="smoothing", corner_smoothing=0.15,
                 multigrid="none", check_every=64, graph_iters=16,
                 persistent=self.mode if self.persistent is None else self.persistent)
        d.update(self.kw)
        return d


def _lone_cases():
    c = []
    for N in (20, 48, 96, 100):                                   # 48, 96: the host's tail layout, T = 3 and 6
        c.append(Case(f"m0-N{N}", 0, N, Re=100.0 if N < 50 else 400.0))
    for N in (16, 24, 47, 64, 79):                                # one tile with all three index-(M-1) jobs ... 25 tiles
        c.append(Case(f"m3-N{N}", 3, N, Re=100.0 if N < 50 else 400.0))
    # M = 81 is past the 5 x 5 tiles of an XCD: persistent=3 falls back to the launch path (the tail layout at T = 5)
    c.append(Case("m3-N80-falls-back", 0, 80, persistent=3))
    for N in (15, 16, 32, 43):                                    # 32: M = 33, the special wave layout; 43: the LDS limit
        for diag in (True, False):
            c.append(Case(f"m4-N{N}-{'diag' if diag else 'step'}", 4, N, Re=100.0, diagnostics=diag))
    for N, layout in ((81, None), (96, "tail"), (96, "tiles"), (112, "tail"), (128, "tail"), (128, "tiles"), (200, None),
                      (255, None), (256, "tail")):
        c.append(Case(f"m5-N{N}" + (f"-{layout}" if layout else ""), 5, N, Re=1000.0 if N > 128 else 400.0, layout=layout))
    for mode, N in ((3, 16), (3, 64), (4, 15), (4, 40), (5, 96), (5, 128)):
        c.append(Case(f"smoother-m{mode}-N{N}", mode, N, Re=1000.0, smoother=True, diagnostics=False))
    for nx, ny in ((24, 40), (40, 20)):
        for mode in (0, 3):
            c.append(Case(f"m{mode}-{nx}x{ny}", mode, nx, ny=ny, Re=100.0))
    for nx, ny in ((48, 129), (129, 48)):                         # 129 x 48: the nx > ny orientation
        c.append(Case(f"m5-{nx}x{ny}", 5, nx, ny=ny, Re=100.0))
    c.append(Case("params-m0-N48-saad", 0, 48, Re=250.0, kw=SAAD))
    for layout in ("tail", "tiles"):
        c.append(Case(f"params-m5-N96-saad-{layout}", 5, 96, Re=250.0, layout=layout, kw=SAAD))
    c.append(Case("params-m3-N24", 3, 24, Re=250.0, kw=PARAMS))
    c.append(Case("params-m4-N20", 4, 20, Re=250.0, kw=PARAMS))
    return [replace(k, seed=1000 + q) for q, k in enumerate(c)]


CASES = _lone_cases()

# a seed that breaks the boundary conditions: nonzero u and v on all four edges, no apply_bc.  Run where index M-1 lies inside
# the tiles (the first residual sees the state as uploaded, every stage imposes the boundary values, like the oracle) ...
RAW_CASES = [Case("raw-m4-N15", 4, 15, Re=100.0, K=3, seed=2001, bc=False),
             Case("raw-m0-N100", 0, 100, K=3, seed=2003, bc=False),
             Case("raw-m5-N100", 5, 100, K=3, seed=2004, bc=False)]
# ... and refused in the host's tail layout, where the kernels take index M-1 of phi^n for boundary values (SGSolver.set_state)
RAW_REFUSED = [Case("raw-m3-N16", 3, 16, Re=100.0, K=3, seed=2000, bc=False),
               Case("raw-m5-N96-tail", 5, 96, K=3, seed=2002, bc=False, layout="tail")]

# seeded N = 128: 3 iterations chip-wide, 2 on the launch path, 3 chip-wide -- one oracle run of 8
HANDOVER = Case("handover-N128", 5, 128, K=8, seed=3000)


@dataclass(frozen=True)
class BatchCase:
    """B trials of one size, each with its own seed and its own Re, advanced together by the batch form of ``mode``."""
    id: str
    mode: int
    N: int
    B: int
    K: int = 4

    def trial(self, q):
        return Case(f"{self.id}[{q}]", self.mode, self.N, Re=100.0 + 7.0 * (q % 40), K=self.K, seed=4000 + 1000 * self.mode + q)


BATCHES = [BatchCase("batch-m0-N48", 0, 48, 3),           # the shared launches of the launch path
           BatchCase("batch-m3-N32", 3, 32, 10),          # more trials than XCDs
           BatchCase("batch-m4-N16", 4, 16, 260),         # more than one 256-trial launch
           BatchCase("batch-m5-N96", 5, 96, 8)]           # two launch groups: 7 and 1


def cpu_cases():
    """Every distinct oracle configuration of the GPU matrix (the first and the last trial stand for a batch)."""
    out = CASES + RAW_CASES + [HANDOVER]
    for b in BATCHES:
        out += [b.trial(0), b.trial(b.B - 1)]
    return out
