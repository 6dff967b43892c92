"""Python host mirror of the reference octree-mg API (``m_octree_mg``).

Same names, argument meaning and error behaviour as the Fortran library the
reference's tests call (tests/test_uniform_grid.f90:77-105):

    mg = MG()                                # type(mg_t) :: mg
    mg.smoother_type = MG_SMOOTHER_GSRB
    mg.bc[nb][MG_IPHI] = BC(MG_BC_DIRICHLET, 0.0)   # or .boundary_cond = f
    mg_set_methods(mg)
    mg_comm_init(mg)
    mg_build_rectangle(mg, domain_size, box_size, dr, r_min, periodic, n_finer)
    mg_load_balance(mg)
    mg_allocate_storage(mg)                  # device arenas live here
    mg_fas_vcycle(mg) / mg_fas_fmg(mg, have_guess, max_res=True)

Host-side tree bookkeeping runs in tree.py; every per-level step runs as HIP
kernels in libomg.so through the C-ABI (device.py).  Box data is exchanged
per level as arrays [box, k, j, i] of the reference's cc(0:nc+1,...) layout.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import device
from .tree import (MG_AHELMHOLTZ, MG_VHELMHOLTZ, MG_VLAPLACIAN, MG_BC_DIRICHLET, MG_CARTESIAN, MG_HELMHOLTZ,
                   MG_IPHI, MG_LAPLACIAN, MG_NO_BOX, MG_NUM_VARS,
                   MG_SMOOTHER_GS, MG_SMOOTHER_GSRB, MGLevel, MGTree)


class BC:
    """mg_bc_t (reference: src/m_data_structures.f90:235-242)."""

    def __init__(self, bc_type=MG_BC_DIRICHLET, bc_value=0.0, boundary_cond=None, refinement_bnd=None):
        self.bc_type = bc_type
        self.bc_value = bc_value
        # boundary_cond(mg, id, nc, iv, nb) -> (bc_type, values[nc*nc], first index fastest)
        self.boundary_cond = boundary_cond
        # refinement_bnd(mg, id, nc, iv, nb, cgc, cc): mg_subr_rb (:364-378);
        # cgc [c-1, a-1] the coarse face (box_gc_for_fine_neighbor), cc
        # [k, j, i] (0..nc+1) the box's variable iv, whose face-nb ghosts it
        # sets in place (omg_set_refinement_bnd: called after every ghost fill)
        self.refinement_bnd = refinement_bnd


# omg_rb_fn (include/omg.h)
_RB_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int),
                     C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double))


def dense_strides(t, what="dense"):
    """(n, stride) in x, y, z order, in elements, of a tensor [nz, ny, nx] as
    omg_put_dense / omg_get_dense take them, or ValueError: the last stride
    must be 1, rows and planes in order and apart (no transposed, expanded or
    overlapping view).  The stride of a dimension of size 1 is arbitrary in
    torch, so it becomes the dense one."""
    n = (t.shape[2], t.shape[1], t.shape[0])
    sx = t.stride(2) if n[0] > 1 else 1
    sy = t.stride(1) if n[1] > 1 else max(sx * n[0], 1)
    sz = t.stride(0) if n[2] > 1 else max(sy * n[1], 1)
    if t.numel():
        if sx != 1:
            raise ValueError(f"{what}: the last stride is {sx}, 1 is required")
        if sy < n[0] or sz < sy * n[1]:
            raise ValueError(f"{what}: strides {tuple(t.stride())} of shape {tuple(t.shape)}: "
                             "stride(1) >= nx and stride(0) >= stride(1) * ny are required")
    return n, (1, sy, sz)


class MG(MGTree):
    """mg_t: tree (host) + device context (HIP)."""

    def __init__(self):
        super().__init__()
        self.is_allocated = False
        self.n_extra_vars = 0
        self.comm = None
        self.operator_type = MG_LAPLACIAN
        self.geometry_type = MG_CARTESIAN
        self.n_smoother_substeps = 1
        self.n_cycle_down = 2
        self.n_cycle_up = 2
        self.max_coarse_cycles = 1000
        self.residual_coarse_abs = 1e-8
        self.residual_coarse_rel = 1e-8
        self.helmholtz_lambda = 0.0
        self.methods_set = False
        self.bc = [[BC() for _ in range(17)] for _ in range(7)]   # bc[nb][iv], 1-based
        self.ctx: device.Context | None = None
        self.device_index = 0
        self._uid = None
        # replicate coarse levels of up to this many cells on every rank
        # (omg_set_coarse_replication; 0 = split them like the reference)
        self.coarse_replication_cells = 0

    # -- data access -------------------------------------------------------
    @property
    def n_vars(self):
        return MG_NUM_VARS + self.n_extra_vars

    def set_level(self, lvl, iv, data):
        """Upload variable iv of all my_ids boxes at lvl ([box, k, j, i])."""
        self._require_alloc()
        self.ctx.upload_level(lvl, iv, data)

    def get_level(self, lvl, iv):
        self._require_alloc()
        return self.ctx.download_level(lvl, iv)

    @staticmethod
    def _dense_layout(t, what):
        """The type, dtype and stride checks of a tensor [nz, ny, nx]; returns
        (n, stride) in x, y, z order."""
        import torch
        if not isinstance(t, torch.Tensor) or t.dim() != 3:
            raise ValueError(f"{what}: a torch tensor [nz, ny, nx] is required")
        if t.dtype != torch.float64:
            raise ValueError(f"{what}: dtype {t.dtype}, torch.float64 is required")
        return dense_strides(t, what)

    def _dense_args(self, t, what):
        """The checks of set_dense / get_dense on a tensor [nz, ny, nx], before
        any call into the library; returns (n, stride) in x, y, z order."""
        n, stride = self._dense_layout(t, what)
        if not t.is_cuda:
            raise ValueError(f"{what}: the tensor is on {t.device}, not on the context's GPU")
        self._require_alloc()
        dev = self.ctx.device
        if dev >= 0 and t.device.index != dev:
            raise ValueError(f"{what}: the tensor is on {t.device}, the context on GPU {dev}")
        return n, stride

    def level_grid(self, lvl):
        """(nx, ny, nz): the cell grid of level lvl over the whole domain."""
        return tuple(int(v) for v in self.domain_size_lvl[lvl])

    def set_dense(self, lvl, iv, tensor, lo=(0, 0, 0)):
        """omg_put_dense: the torch.float64 tensor [nz, ny, nx] on the context's
        GPU (the last stride 1, rows and planes in order and not
        overlapping: stride(1) >= nx, stride(0) >= stride(1) * ny) is the window of level lvl's cell
        grid that starts at the 0-based cell lo = (x, y, z); the interior cells
        of this rank's boxes inside it take its values, ghost cells and cells
        outside keep theirs.  Ordered on torch's current stream: no host
        synchronisation.  Returns the number of cells copied."""
        import torch
        n, stride = self._dense_args(tensor, "set_dense")
        return self.ctx.put_dense(lvl, iv, tensor.data_ptr(), lo, n, stride,
                                  torch.cuda.current_stream(tensor.device).cuda_stream)

    def get_dense(self, lvl, iv, out=None, lo=(0, 0, 0), shape=None):
        """omg_get_dense into `out` [nz, ny, nx] (default: torch.empty of
        shape = (nz, ny, nx), the level's whole cell grid from lo when None).
        Elements that no box of this rank covers keep their values.  Returns
        (out, cells copied)."""
        import torch
        if out is None:
            self._require_alloc()
            if shape is None:
                g = self.level_grid(lvl)
                shape = tuple(max(g[2 - q] - int(lo[2 - q]), 0) for q in range(3))
            dev = self.ctx.device
            out = torch.empty(tuple(int(v) for v in shape), dtype=torch.float64,
                              device=torch.device("cuda", dev if dev >= 0 else torch.cuda.current_device()))
        n, stride = self._dense_args(out, "get_dense")
        cells = self.ctx.get_dense(lvl, iv, out.data_ptr(), lo, n, stride,
                                   torch.cuda.current_stream(out.device).cuda_stream)
        return out, cells

    def get_dense_grad(self, lvl, iv=1, out=None, lo=(0, 0, 0), shape=None, scale=1.0, fill=True,
                       components=(True, True, True)):
        """omg_get_dense_grad: the central differences of variable iv at lvl,
        component d = (cc(+1 in d) - cc(-1 in d)) * 0.5 * scale / dr_d over the
        boxes and their ghost cells (scale = -1.0: the field of a potential),
        as dense windows that start at the 0-based cell lo = (x, y, z).
        `out` is a torch.float64 tensor [3, nz, ny, nx] on the context's GPU
        (x, y, z components; default: torch.empty of shape = (nz, ny, nx), the
        level's whole cell grid from lo when None), or a sequence of three
        tensors [nz, ny, nx] or Nones of one shape and one set of strides; the
        layout checks are set_dense's.  A component that is None or whose entry
        of `components` is false is skipped and its tensor left untouched.
        fill: the ghost cells of iv at lvl are filled first (collective on
        several ranks); without it they are used as they stand.  Elements that
        no box of this rank covers keep their values.  Ordered on torch's
        current stream.  Returns (out, cells covered)."""
        import torch
        what = "get_dense_grad"
        if len(components) != 3:
            raise ValueError(f"{what}: components takes three flags")
        if out is None:
            self._require_alloc()
            if shape is None:
                g = self.level_grid(lvl)
                shape = tuple(max(g[2 - q] - int(lo[2 - q]), 0) for q in range(3))
            dev = self.ctx.device
            out = torch.empty((3,) + tuple(int(v) for v in shape), dtype=torch.float64,
                              device=torch.device("cuda", dev if dev >= 0 else torch.cuda.current_device()))
        if isinstance(out, torch.Tensor):
            if out.dim() != 4 or out.shape[0] != 3:
                raise ValueError(f"{what}: a torch tensor [3, nz, ny, nx] is required")
            parts = [out[d] for d in range(3)]
        else:
            parts = list(out)
            if len(parts) != 3:
                raise ValueError(f"{what}: three tensors (or None) are required")
        parts = [t if components[d] else None for d, t in enumerate(parts)]
        used = [t for t in parts if t is not None]
        if not used:
            raise ValueError(f"{what}: no component is asked for")
        layouts = [self._dense_layout(t, what) for t in used]
        if any(a != layouts[0] for a in layouts):
            raise ValueError(f"{what}: the components differ in shape or strides")
        for t in used:
            self._dense_args(t, what)
        if any(t.device != used[0].device for t in used):
            raise ValueError(f"{what}: the components are on different devices")
        n, stride = layouts[0]
        cells = self.ctx.get_dense_grad(lvl, iv, [0 if t is None else t.data_ptr() for t in parts], lo, n, stride,
                                        scale, fill, torch.cuda.current_stream(used[0].device).cuda_stream)
        return out, cells

    def _blocks_args(self, t, ids, ghost_width, ghosts, what):
        """The checks of set_blocks / get_blocks on a tensor [n, m, m, m], before
        any call into the library; returns (ids, box_off, stride, nc)."""
        import torch
        ghost_width = int(ghost_width)
        if ghost_width < 0:
            raise ValueError(f"{what}: ghost_width {ghost_width} < 0")
        if ghosts and ghost_width < 1:
            raise ValueError(f"{what}: ghosts=True needs ghost_width >= 1")
        if not isinstance(t, torch.Tensor) or t.dim() != 4:
            raise ValueError(f"{what}: a torch tensor [box, k, j, i] is required")
        if t.dtype != torch.float64:
            raise ValueError(f"{what}: dtype {t.dtype}, torch.float64 is required")
        ids = np.ascontiguousarray(ids, dtype=np.int64).reshape(-1)
        n = int(t.shape[0])
        if len(ids) != n:
            raise ValueError(f"{what}: {len(ids)} ids for {n} blocks")
        if n and (ids.min() < 1 or ids.max() > self.n_boxes):
            raise ValueError(f"{what}: a box id outside 1..{self.n_boxes}")
        sizes = {int(self.box_size_lvl[int(l)]) for l in np.unique(self.lvl[ids])} if n else set()
        if len(sizes) > 1:
            raise ValueError(f"{what}: the listed boxes have the box sizes {sorted(sizes)}, one is required")
        m = int(t.shape[3])
        nc = sizes.pop() if sizes else m - 2 * ghost_width
        if tuple(t.shape[1:]) != (nc + 2 * ghost_width,) * 3:
            raise ValueError(f"{what}: blocks of shape {tuple(t.shape[1:])}, box size {nc} with ghost_width "
                             f"{ghost_width} needs {(nc + 2 * ghost_width,) * 3}")
        sb, s2, s1, s0 = (int(v) for v in t.stride())
        if n and m:
            if s0 != 1:
                raise ValueError(f"{what}: the last stride is {s0}, 1 is required")
            if s1 < m or s2 < s1 * m or sb < 0:
                raise ValueError(f"{what}: strides {tuple(t.stride())} of shape {tuple(t.shape)}: stride(2) >= m, "
                                 "stride(1) >= stride(2) * m and stride(0) >= 0 are required")
        if not t.is_cuda:
            raise ValueError(f"{what}: the tensor is on {t.device}, not on the context's GPU")
        self._require_alloc()
        dev = self.ctx.device
        if dev >= 0 and t.device.index != dev:
            raise ValueError(f"{what}: the tensor is on {t.device}, the context on GPU {dev}")
        box_off = np.arange(n, dtype=np.int64) * sb + ghost_width * (1 + s1 + s2)
        return ids.astype(np.int32), box_off, (1, max(s1, 1), max(s2, 1)), nc

    def set_blocks(self, iv, blocks, ids, ghost_width=0, ghosts=False):
        """omg_put_boxes: variable iv of the boxes `ids` (1-based global ids of
        this rank, in any order, on any levels that share one box size nc) from
        `blocks`, a torch.float64 tensor [n, m, m, m] ([box, k, j, i]) on the
        context's GPU with m = nc + 2 * ghost_width: the block pool of an AMR
        code with ghost_width ghost layers of its own.  The last stride is 1,
        stride(2) >= m, stride(1) >= stride(2) * m and the box stride is any
        value >= 0: a slice pool[:, iw] of a pool [n, nw, m, m, m] is a valid
        argument.  The interiors move; ghosts=True (ghost_width >= 1): also
        the innermost ghost layer on the six faces, as set_level's ghosts.
        Edges, corners and outer ghost layers are never read.  Ordered on
        torch's current stream: no host synchronisation.  With several ranks
        a put of phi is collective (a rank with nothing passes n = 0).
        Returns the number of cells copied."""
        import torch
        ids, off, stride, _ = self._blocks_args(blocks, ids, ghost_width, ghosts, "set_blocks")
        return self.ctx.put_boxes(iv, ids, blocks.data_ptr(), off, stride, int(bool(ghosts)),
                                  torch.cuda.current_stream(blocks.device).cuda_stream)

    def get_blocks(self, iv, ids, out=None, ghost_width=0, ghosts=False, fill=True):
        """omg_get_boxes into `out` [n, m, m, m] (default: torch.empty of that
        shape), laid out as set_blocks' tensor.  ghosts=True: with the
        innermost ghost layer on the six faces; edges, corners and everything
        else of `out` outside the copied cells keep their values.  fill: the
        ghost cells of iv are filled first on every level (collective on
        several ranks); without it they are used as they stand.  Returns
        (out, cells copied)."""
        import torch
        if out is None:
            self._require_alloc()
            idl = np.ascontiguousarray(ids, dtype=np.int64).reshape(-1)
            sizes = {int(self.box_size_lvl[int(l)]) for l in np.unique(self.lvl[idl])} if len(idl) else {0}
            if len(sizes) > 1:
                raise ValueError(f"get_blocks: the listed boxes have the box sizes {sorted(sizes)}, one is required")
            m = sizes.pop() + 2 * int(ghost_width)
            dev = self.ctx.device
            out = torch.empty((len(idl), m, m, m), dtype=torch.float64,
                              device=torch.device("cuda", dev if dev >= 0 else torch.cuda.current_device()))
        ids, off, stride, _ = self._blocks_args(out, ids, ghost_width, ghosts, "get_blocks")
        cells = self.ctx.get_boxes(iv, ids, out.data_ptr(), off, stride, int(bool(ghosts)), fill,
                                   torch.cuda.current_stream(out.device).cuda_stream)
        return out, cells

    def get_blocks_grad(self, ids, iv=1, out=None, ghost_width=0, scale=1.0, fill=True, centering="cell",
                        components=(True, True, True)):
        """omg_get_boxes_grad: the gradient of variable iv over the boxes `ids`
        (as get_blocks lists them) in block layout.  `out` is a torch.float64
        tensor [3, n, m, m, m] on the context's GPU (x, y, z components,
        m = nc + 2 * ghost_width; default: torch.empty of that shape), or a
        sequence of three tensors [n, m, m, m] or Nones of one shape and one
        set of strides; the layout checks are set_blocks'.  A component that
        is None or whose entry of `components` is false is skipped and its
        tensor left untouched.
        centering="cell": (cc(+1 in d) - cc(-1 in d)) * 0.5 * scale / dr_d at
        the interior cells of each block (get_dense_grad's values).
        centering="face" (ghost_width >= 1): (cc(+1 in d) - cc) * scale / dr_d
        for the index along d from 0 to nc, face i at cell i's element, so
        face 0 lies in the first ghost layer below the interior.
        scale = -1.0: the field of a potential.  fill: the ghost cells of iv
        are filled first on every level (collective on several ranks), so that
        refinement-boundary ghosts carry the coarse neighbour's interpolation;
        without it they are used as they stand.  Everything else of `out`
        keeps its values.  Ordered on torch's current stream.  Returns
        (out, values per component)."""
        import torch
        what = "get_blocks_grad"
        if centering not in ("cell", "face"):
            raise ValueError(f"{what}: centering {centering!r}, 'cell' or 'face' is required")
        if len(components) != 3:
            raise ValueError(f"{what}: components takes three flags")
        if centering == "face" and int(ghost_width) < 1:
            raise ValueError(f"{what}: centering='face' needs ghost_width >= 1")
        if out is None:
            self._require_alloc()
            idl = np.ascontiguousarray(ids, dtype=np.int64).reshape(-1)
            sizes = {int(self.box_size_lvl[int(l)]) for l in np.unique(self.lvl[idl])} if len(idl) else {0}
            if len(sizes) > 1:
                raise ValueError(f"{what}: the listed boxes have the box sizes {sorted(sizes)}, one is required")
            m = sizes.pop() + 2 * int(ghost_width)
            dev = self.ctx.device
            out = torch.empty((3, len(idl), m, m, m), dtype=torch.float64,
                              device=torch.device("cuda", dev if dev >= 0 else torch.cuda.current_device()))
        if isinstance(out, torch.Tensor):
            if out.dim() != 5 or out.shape[0] != 3:
                raise ValueError(f"{what}: a torch tensor [3, box, k, j, i] is required")
            parts = [out[d] for d in range(3)]
        else:
            parts = list(out)
            if len(parts) != 3:
                raise ValueError(f"{what}: three tensors (or None) are required")
        parts = [t if components[d] else None for d, t in enumerate(parts)]
        used = [t for t in parts if t is not None]
        if not used:
            raise ValueError(f"{what}: no component is asked for")
        args = [self._blocks_args(t, ids, ghost_width, False, what) for t in used]
        idl, off, stride, _ = args[0]
        if any(t.shape != used[0].shape or t.stride() != used[0].stride() for t in used):
            raise ValueError(f"{what}: the components differ in shape or strides")
        if any(t.device != used[0].device for t in used):
            raise ValueError(f"{what}: the components are on different devices")
        cells = self.ctx.get_boxes_grad(iv, idl, [0 if t is None else t.data_ptr() for t in parts], off, stride,
                                        scale, int(centering == "face"), fill,
                                        torch.cuda.current_stream(used[0].device).cuda_stream)
        return out, cells

    def flux_coefficients(self, coef=None):
        """The coefficient variables (x, y, z; 0: none) get_blocks_flux uses.
        coef=None: the operator's own, by operator_type: none for the
        Laplacian and Helmholtz operators, (5, 5, 5) for the variable-
        coefficient ones (eps in variable 5), (5, 6, 7) for the anisotropic
        one.  Otherwise one variable for all three components, or a sequence
        of three, 0 or None meaning none."""
        if coef is None:
            if self.operator_type in (MG_VLAPLACIAN, MG_VHELMHOLTZ):
                return (5, 5, 5)
            if self.operator_type == MG_AHELMHOLTZ:
                return (5, 6, 7)
            if self.operator_type in (MG_LAPLACIAN, MG_HELMHOLTZ):
                return (0, 0, 0)
            raise ValueError("get_blocks_flux: unknown operator")
        if isinstance(coef, (int, np.integer)) and not isinstance(coef, bool):
            return (int(coef),) * 3
        try:
            vals = tuple(0 if v is None else int(v) for v in coef)
        except TypeError:
            raise ValueError(f"get_blocks_flux: coef {coef!r}, a variable or a sequence of three is required") from None
        if len(vals) != 3:
            raise ValueError("get_blocks_flux: coef takes one variable or three")
        return vals

    def get_blocks_flux(self, ids, iv=1, coef=None, out=None, ghost_width=0, scale=1.0, fill=True, centering="face",
                        accumulate=False, components=(True, True, True)):
        """omg_get_boxes_flux: get_blocks_grad's values, each component
        weighted by a coefficient variable and optionally added to `out`;
        `out`, its forms and its layout checks are get_blocks_grad's.  With g
        the gradient's value of an element:
        centering="face" (the default; ghost_width >= 1): v = c * g with
        c = ((2 * a_lo) * a_hi) / (a_lo + a_hi), the harmonic mean of the
        coefficient in the face's two cells, the face weight of the operators
        with a cell coefficient, so that the face-centred divergence of the
        result (set_blocks_div) is what the solver inverted; the coefficient's
        face ghosts are read as they stand.  centering="cell": v = a * g with
        the cell's own coefficient.  A component without a coefficient: v = g.
        coef: see flux_coefficients; None takes the operator's own.
        accumulate=True: out = out + v (out is required), e.g. scale=-1.0 for
        the correction B -= grad(phi) of a projection in one pass.  fill: the
        ghost cells of iv are filled first on every level (collective on
        several ranks); the coefficients are never filled.  Ordered on torch's
        current stream.  Returns (out, values per component)."""
        import torch
        what = "get_blocks_flux"
        if centering not in ("cell", "face"):
            raise ValueError(f"{what}: centering {centering!r}, 'cell' or 'face' is required")
        if len(components) != 3:
            raise ValueError(f"{what}: components takes three flags")
        if centering == "face" and int(ghost_width) < 1:
            raise ValueError(f"{what}: centering='face' needs ghost_width >= 1")
        if accumulate and out is None:
            raise ValueError(f"{what}: accumulate=True needs `out`")
        iv_coef = self.flux_coefficients(coef)
        n_vars = self.n_vars
        for v in iv_coef:
            if v < 0 or v > n_vars or v == iv:
                raise ValueError(f"{what}: coefficient variable {v}: 0 or a variable 1..{n_vars} other than iv = {iv} "
                                 "is required")
        if out is None:
            self._require_alloc()
            idl = np.ascontiguousarray(ids, dtype=np.int64).reshape(-1)
            sizes = {int(self.box_size_lvl[int(l)]) for l in np.unique(self.lvl[idl])} if len(idl) else {0}
            if len(sizes) > 1:
                raise ValueError(f"{what}: the listed boxes have the box sizes {sorted(sizes)}, one is required")
            m = sizes.pop() + 2 * int(ghost_width)
            dev = self.ctx.device
            out = torch.empty((3, len(idl), m, m, m), dtype=torch.float64,
                              device=torch.device("cuda", dev if dev >= 0 else torch.cuda.current_device()))
        if isinstance(out, torch.Tensor):
            if out.dim() != 5 or out.shape[0] != 3:
                raise ValueError(f"{what}: a torch tensor [3, box, k, j, i] is required")
            parts = [out[d] for d in range(3)]
        else:
            parts = list(out)
            if len(parts) != 3:
                raise ValueError(f"{what}: three tensors (or None) are required")
        parts = [t if components[d] else None for d, t in enumerate(parts)]
        used = [t for t in parts if t is not None]
        if not used:
            raise ValueError(f"{what}: no component is asked for")
        args = [self._blocks_args(t, ids, ghost_width, False, what) for t in used]
        idl, off, stride, _ = args[0]
        if any(t.shape != used[0].shape or t.stride() != used[0].stride() for t in used):
            raise ValueError(f"{what}: the components differ in shape or strides")
        if any(t.device != used[0].device for t in used):
            raise ValueError(f"{what}: the components are on different devices")
        cells = self.ctx.get_boxes_flux(iv, iv_coef, idl, [0 if t is None else t.data_ptr() for t in parts], off,
                                        stride, scale, int(centering == "face"), bool(accumulate), fill,
                                        torch.cuda.current_stream(used[0].device).cuda_stream)
        return out, cells

    def set_blocks_div(self, iv, blocks, ids, ghost_width, scale=1.0, centering="cell",
                       components=(True, True, True)):
        """omg_put_boxes_div: variable iv of the boxes `ids` (as set_blocks lists
        them) becomes the divergence of the vector field in `blocks`, a
        torch.float64 tensor [3, n, m, m, m] on the context's GPU (x, y, z
        components, m = nc + 2 * ghost_width), or a sequence of three tensors
        [n, m, m, m] or Nones of one shape and one set of strides; the layout
        checks are get_blocks_grad's, and since nothing is written the
        components may be one and the same tensor.  A component that is None
        or whose entry of `components` is false is skipped and never read.
        ghost_width >= 1: both centrings read the first ghost layer.
        centering="cell": the sum over the components, in the order x, y, z,
        of (V_d(+1 in d) - V_d(-1 in d)) * 0.5 * scale / dr_d with V_d at the
        cells: the interior and the innermost ghost layer on the six faces are
        read.  centering="face": of (V_d - V_d(-1 in d)) * scale / dr_d with
        V_d(i) on the face between the cells i and i+1 along d, the layout
        get_blocks_grad(centering="face") writes: the index along d from 0 to
        nc is read.  Edges, corners and outer ghost layers are never read;
        the ghost cells of iv keep their values.  Ordered on torch's current
        stream: no host synchronisation.  With several ranks a call for phi
        is collective (a rank with nothing passes n = 0).  Returns the number
        of cells written."""
        import torch
        what = "set_blocks_div"
        if centering not in ("cell", "face"):
            raise ValueError(f"{what}: centering {centering!r}, 'cell' or 'face' is required")
        if len(components) != 3:
            raise ValueError(f"{what}: components takes three flags")
        if int(ghost_width) < 1:
            raise ValueError(f"{what}: ghost_width >= 1 is required")
        if isinstance(blocks, torch.Tensor):
            if blocks.dim() != 5 or blocks.shape[0] != 3:
                raise ValueError(f"{what}: a torch tensor [3, box, k, j, i] is required")
            parts = [blocks[d] for d in range(3)]
        else:
            parts = list(blocks)
            if len(parts) != 3:
                raise ValueError(f"{what}: three tensors (or None) are required")
        parts = [t if components[d] else None for d, t in enumerate(parts)]
        used = [t for t in parts if t is not None]
        if not used:
            raise ValueError(f"{what}: no component is given")
        args = [self._blocks_args(t, ids, ghost_width, False, what) for t in used]
        idl, off, stride, _ = args[0]
        if any(t.shape != used[0].shape or t.stride() != used[0].stride() for t in used):
            raise ValueError(f"{what}: the components differ in shape or strides")
        if any(t.device != used[0].device for t in used):
            raise ValueError(f"{what}: the components are on different devices")
        return self.ctx.put_boxes_div(iv, idl, [0 if t is None else t.data_ptr() for t in parts], off, stride,
                                      scale, int(centering == "face"),
                                      torch.cuda.current_stream(used[0].device).cuda_stream)

    def _require_alloc(self):
        if not self.is_allocated:
            raise RuntimeError("allocate_storage: tree is not allocated")

    # -- device configuration (mg_set_methods) ---------------------------
    def _push_methods(self):
        c = self.ctx
        c.call("set_operator", self.operator_type, float(self.helmholtz_lambda))
        c.call("set_smoother", self.smoother_type, self.n_cycle_down, self.n_cycle_up,
               self.max_coarse_cycles, self.residual_coarse_abs, self.residual_coarse_rel)
        c.call("set_subtract_mean", int(self.subtract_mean))

    def _rb_trampoline(self, iv, nb, cb):
        def fn(user, lvl, iv_, n, ids, nbs, nc, cgc, cc):
            try:
                s = nc + 2
                g = np.ctypeslib.as_array(cgc, shape=(n, nc, nc))
                a = np.ctypeslib.as_array(cc, shape=(n, s, s, s))
                for q in range(n):
                    cb(self, int(ids[q]), nc, iv_, int(nbs[q]), g[q], a[q])
            except BaseException as ex:  # noqa: BLE001  (no exception may cross the C frame)
                self._rb_error = ex
        return _RB_FN(fn)

    def _raise_rb_error(self):
        ex = getattr(self, "_rb_error", None)
        if ex is not None:
            self._rb_error = None
            raise ex

    def push_bc(self, ivs=None):
        """Send mg%bc to the device; boundary_cond callbacks are tabulated per
        physical face of my boxes (they are pure functions of box geometry);
        refinement_bnd callbacks are handed to omg_set_refinement_bnd."""
        c = self.ctx
        ivs = range(1, self.n_vars + 1) if ivs is None else ivs
        if not hasattr(self, "_rb_keep"):
            self._rb_keep = {}
            c.after_call = self._raise_rb_error
        for iv in ivs:
            for nb in range(1, 7):
                cb = self.bc[nb][iv].refinement_bnd
                had = self._rb_keep.get((iv, nb)) is not None
                fp = self._rb_keep[(iv, nb)] = self._rb_trampoline(iv, nb, cb) if cb else None
                if fp or had:   # (nothing to clear otherwise: older libraries lack the entry)
                    c.call("set_refinement_bnd", iv, nb, C.cast(fp, C.c_void_p) if fp else None, None)
            cbs = [self.bc[nb][iv].boundary_cond for nb in range(1, 7)]
            for nb in range(1, 7):
                b = self.bc[nb][iv]
                c.call("set_bc", iv, nb, int(b.bc_type), float(b.bc_value))
            if any(cb is not None for cb in cbs):
                n = self.n_boxes
                face_off = np.full(n * 6, -1, dtype=np.int64)
                face_type = np.zeros(n * 6, dtype=np.int32)
                chunks, pos = [], 0
                rep = c.replicated_level()
                for lvl in range(self.lowest_lvl, self.highest_lvl + 1):
                    nc = self.box_size_lvl[lvl]
                    # a replicated level needs the table of every box
                    for id_ in (self.lvls[lvl].ids if lvl <= rep else self.lvls[lvl].my_ids):
                        for nb in range(1, 7):
                            if self.neighbors[id_, nb - 1] < MG_NO_BOX and cbs[nb - 1] is not None:
                                t, vals = cbs[nb - 1](self, int(id_), nc, iv, nb)
                                vals = np.ascontiguousarray(vals, dtype=np.float64).reshape(-1)
                                face_off[(id_ - 1) * 6 + nb - 1] = pos
                                face_type[(id_ - 1) * 6 + nb - 1] = t
                                chunks.append(vals)
                                pos += vals.size
                data = np.concatenate(chunks) if chunks else np.zeros(1)
                c.call("set_bc_faces", iv, face_off, face_type, data, len(data))


# ---------------------------------------------------------------------------
# The public procedures (names as in the reference's m_octree_mg)

class Loopback:
    """Communicator of an in-process loopback group: n_ranks MG objects of one
    process, one host thread each, sharing a GPU (include/omg.h,
    omg_loopback_unique_id).  Used to run the multi-rank path on one GPU."""

    def __init__(self, tag: int, rank: int, n_ranks: int):
        self.tag, self.rank, self.n_ranks = int(tag), int(rank), int(n_ranks)


def mg_comm_init(mg: MG, comm=None):
    """mg_comm_init (reference: src/m_communication.f90:14-35).  Ranks come
    from torch.distributed when it is initialised (or from a Loopback
    communicator), else a single rank."""
    if isinstance(comm, Loopback):
        mg.comm, mg.my_rank, mg.n_cpu = comm, comm.rank, comm.n_ranks
        return
    try:
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized():
            mg.comm = comm or dist.group.WORLD
            mg.my_rank = dist.get_rank()
            mg.n_cpu = dist.get_world_size()
            return
    except ImportError:
        pass
    mg.comm = None
    mg.my_rank = 0
    mg.n_cpu = 1


def mg_set_methods(mg: MG):
    """mg_set_methods (reference: src/m_multigrid.f90:27-60)."""
    if mg.operator_type == MG_LAPLACIAN:
        if np.all(mg.periodic):
            mg.subtract_mean = True
    elif mg.operator_type == MG_HELMHOLTZ:
        mg.subtract_mean = False
    elif mg.operator_type in (MG_VLAPLACIAN, MG_VHELMHOLTZ):
        # vlaplacian_set_methods / vhelmholtz_set_methods (m_vlaplacian.f90:13-49,
        # m_vhelmholtz.f90:19-49): eps in var 5 with Neumann-0 ghosts
        mg.n_extra_vars = max(1, mg.n_extra_vars)
        mg.subtract_mean = False
        for nb in range(1, 7):
            mg.bc[nb][5] = BC(-11, 0.0)
    elif mg.operator_type == MG_AHELMHOLTZ:
        mg.n_extra_vars = max(3, mg.n_extra_vars)
        for nb in range(1, 7):
            for iv in (5, 6, 7):
                mg.bc[nb][iv] = BC(-11, 0.0)
    else:
        raise RuntimeError("mg_set_methods: unknown operator")
    if mg.smoother_type not in (MG_SMOOTHER_GS, MG_SMOOTHER_GSRB):
        raise RuntimeError("unsupported smoother type")
    mg.n_smoother_substeps = 2 if mg.smoother_type == MG_SMOOTHER_GSRB else 1
    mg.methods_set = True
    if mg.ctx is not None:
        mg._push_methods()


def helmholtz_set_lambda(mg: MG, lam: float):
    """helmholtz_set_lambda (reference: src/m_helmholtz.f90:39-46)."""
    if lam < 0:
        raise RuntimeError("helmholtz_set_lambda: lambda < 0 not allowed")
    mg.helmholtz_lambda = float(lam)
    if mg.ctx is not None:
        mg._push_methods()


def mg_build_rectangle(mg: MG, domain_size, box_size, dx, r_min, periodic, n_finer=0):
    mg.build_rectangle(domain_size, box_size, dx, r_min, periodic, n_finer)


def mg_load_balance(mg: MG):
    mg.load_balance()


def mg_load_balance_parents(mg: MG):
    mg.load_balance_parents()


def mg_load_balance_simple(mg: MG):
    mg.load_balance_simple()


def mg_add_children(mg: MG, id_):
    mg.add_children(id_)


def _tree_arrays(mg: MG):
    n = mg.n_boxes
    i32 = lambda a: np.ascontiguousarray(np.asarray(a)[1:n + 1], dtype=np.int32).reshape(-1)
    lo, hi = mg.lowest_lvl, mg.highest_lvl
    bsl = np.array([mg.box_size_lvl[l] for l in range(lo, hi + 1)], dtype=np.int32)
    dr = np.ascontiguousarray(np.array([mg.dr[l] for l in range(lo, hi + 1)],
                                       dtype=np.float64).reshape(-1))
    off, data = [0], []
    for l in range(lo, hi + 1):
        L = mg.lvls[l]
        for arr in (L.ids, L.leaves, L.parents, L.ref_bnds):
            data.extend(int(x) for x in arr)
            off.append(len(data))
    return (i32(mg.lvl), i32(mg.parent), i32(mg.children), i32(mg.neighbors), i32(mg.ix),
            i32(mg.rank), bsl, dr, np.array(off, dtype=np.int32),
            np.array(data if data else [0], dtype=np.int32))


def mg_allocate_storage(mg: MG, device_index=None):
    """mg_allocate_storage (reference: src/m_allocate_storage.f90:51-99): the
    device arenas of every level this rank owns boxes on, zero-initialised."""
    if not mg.tree_created:
        raise RuntimeError("allocate_storage: tree is not yet created")
    if mg.is_allocated:
        raise RuntimeError("allocate_storage: tree is already allocated")
    if device_index is None:
        device_index = int(os.environ.get("LOCAL_RANK", mg.device_index if mg.n_cpu == 1 else 0))
    uid = None
    host = False
    if isinstance(mg.comm, Loopback):
        uid = device.loopback_unique_id(mg.comm.tag) if mg.comm.n_ranks > 1 else None
        device_index = 0
    elif mg.n_cpu > 1:
        import torch.distributed as dist
        host = _use_host_transport(mg)
        if host:
            # ranks share a GPU (RCCL refuses that): the host transport over
            # the torch.distributed group, rank r on GPU r mod ndev
            uid = device.host_unique_id()
            device_index = mg.my_rank % max(device.device_count(), 1)
        else:
            obj = [device.unique_id() if mg.my_rank == 0 else None]
            dist.broadcast_object_list(obj, src=0)
            uid = obj[0]
    mg.ctx = device.Context(device_index, mg.my_rank, mg.n_cpu, uid)
    if host:
        mg.ctx.set_host_transport(mg.comm)
    if mg.coarse_replication_cells:
        mg.ctx.call("set_coarse_replication", int(mg.coarse_replication_cells))
    arrs = _tree_arrays(mg)
    mg.ctx.call("tree_setup", mg.n_boxes, *arrs[:6], mg.lowest_lvl, mg.highest_lvl,
                mg.first_normal_lvl, mg.box_size, arrs[6], arrs[7], arrs[8], arrs[9], mg.n_vars)
    mg.is_allocated = True
    mg._push_methods()
    mg.push_bc()


def _use_host_transport(mg: MG) -> bool:
    """The host transport when this node's ranks outnumber its visible GPUs
    or OMG_TRANSPORT=host; agreed over the group (as the Fortran drop-in
    does).  The node's ranks: LOCAL_WORLD_SIZE (torchrun, bench.py's own
    launcher), else every rank of the group (one node)."""
    import torch
    import torch.distributed as dist
    n_node = int(os.environ.get("LOCAL_WORLD_SIZE", mg.n_cpu))
    want = os.environ.get("OMG_TRANSPORT") == "host" or device.device_count() < n_node
    t = torch.tensor([1 if want else 0], dtype=torch.int64)
    dist.all_reduce(t, op=dist.ReduceOp.MAX, group=mg.comm)
    return bool(t[0])


def mg_deallocate_storage(mg: MG):
    if not mg.is_allocated:
        raise RuntimeError("deallocate_storage: tree is not allocated")
    mg.ctx.close()
    mg.ctx = None
    # as src/m_allocate_storage.f90:14-47: the level lists go, the tree is empty
    for lvl in range(mg.lowest_lvl, mg.highest_lvl + 1):
        mg.lvls[lvl] = MGLevel()
    mg.n_boxes = 0
    mg.is_allocated = False


def _check_methods(mg):
    if not mg.methods_set:
        mg_set_methods(mg)


def mg_fas_vcycle(mg: MG, highest_lvl=None, max_res=False, standalone=True):
    """mg_fas_vcycle (reference: src/m_multigrid.f90:150-243).  Returns the
    max residual when max_res is requested, else None."""
    _check_methods(mg)
    mg._require_alloc()
    hl = mg.lowest_lvl - 1 if highest_lvl is None else int(highest_lvl)
    r = C.c_double(0.0)
    mg.ctx.call("fas_vcycle", hl, int(bool(max_res)), C.byref(r), int(bool(standalone)))
    return r.value if max_res else None


def mg_fas_fmg(mg: MG, have_guess, max_res=False):
    """mg_fas_fmg (reference: src/m_multigrid.f90:84-147)."""
    _check_methods(mg)
    mg._require_alloc()
    r = C.c_double(0.0)
    mg.ctx.call("fas_fmg", int(bool(have_guess)), int(bool(max_res)), C.byref(r))
    return r.value if max_res else None


def mg_apply_op(mg: MG, i_out):
    """mg_apply_op (reference: src/m_multigrid.f90:439-456)."""
    mg.ctx.call("apply_op", i_out)


def mg_restrict(mg: MG, iv):
    mg.ctx.call("restrict", iv)


def mg_restrict_lvl(mg: MG, iv, lvl):
    mg.ctx.call("restrict_lvl", iv, lvl)


def mg_fill_ghost_cells(mg: MG, iv):
    mg.ctx.call("fill_ghost_cells", iv)


def mg_fill_ghost_cells_lvl(mg: MG, lvl, iv):
    mg.ctx.call("fill_ghost_cells_lvl", lvl, iv)


def mg_prolong(mg: MG, lvl, iv, iv_to, add):
    mg.ctx.call("prolong", lvl, iv, iv_to, int(bool(add)))


def mg_set_dense(mg: MG, lvl, iv, tensor, lo=(0, 0, 0)):
    """MG.set_dense (omg_put_dense): a dense device tensor into variable iv."""
    return mg.set_dense(lvl, iv, tensor, lo)


def mg_get_dense(mg: MG, lvl, iv, out=None, lo=(0, 0, 0), shape=None):
    """MG.get_dense (omg_get_dense): variable iv into a dense device tensor."""
    return mg.get_dense(lvl, iv, out, lo, shape)


def mg_phi_bc_store(mg: MG):
    """mg_phi_bc_store (reference: src/m_ghost_cells.f90:66-117): phi's bc
    values move into the rhs ghost cells on the device."""
    mg.ctx.call("phi_bc_store")
    mg.phi_bc_data_stored = True
