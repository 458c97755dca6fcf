"""CPU checks of the owned-block preconditioner (the reference's PCBJACOBI with PCBJacobiSetTotalBlocks(size*nElsX*nElsX)): PETSc's equal
contiguous chunks of the global 1-form numbering are exactly the edges each element owns -- its x-edges of columns 0..n-1 and y-edges of
rows 0..n-1, the rule mimsem_owned_blocks_* read off the element tables -- and the header declares the new entries."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _owned(pn, inds1x, inds1y):
    """per element, the sorted global slots at owned positions (x-edge column < n, y-edge row < n)"""
    n1e = pn * (pn + 1)
    lx = np.arange(n1e)
    ox = lx % (pn + 1) < pn
    oy = lx // pn < pn
    return np.sort(np.concatenate([inds1x[:, ox], inds1y[:, oy]], axis=1), axis=1)


@pytest.mark.parametrize("mesh,pn,ne,npatch", [("sphere", 3, 4, 6), ("sphere", 2, 4, 24), ("sphere", 4, 2, 6), ("sphere", 3, 2, 6),
                                               ("box", 3, 4, 1), ("box", 2, 4, 4)])
def test_chunks_are_owned_edges(mesh, pn, ne, npatch):
    from mimsem_amd.mesh import CubedSphere, PeriodicBox
    from mimsem_amd.topo import Topo
    m = CubedSphere(pn, ne, npatch) if mesh == "sphere" else PeriodicBox(pn, ne, npatch)
    topos = [Topo(m, p, 1) for p in range(npatch)]
    gx = np.concatenate([t.all_inds1x_g() for t in topos])
    gy = np.concatenate([t.all_inds1y_g() for t in topos])
    own = _owned(pn, gx, gy)
    nd = 2 * pn * pn
    nEl = gx.shape[0]
    assert own.shape == (nEl, nd)
    # the owned sets partition the global 1-forms, element k's set is chunk k
    assert nEl * nd == m.nDofs1G
    assert np.array_equal(own.ravel(), np.arange(m.nDofs1G))
    # an edge borders at most two elements (interior edges one): the blocks gather from the owner and at most one neighbour
    cnt = np.bincount(np.concatenate([gx.ravel(), gy.ravel()]), minlength=m.nDofs1G)
    assert ((cnt == 1) | (cnt == 2)).all()


def test_local_numbering_leaves_ghosts_outside_every_block():
    """a rank-local (ghosted) layout: the owned slots of the patch's elements are distinct, and the east / north ghost slots lie in no block"""
    from mimsem_amd.mesh import CubedSphere
    from mimsem_amd.topo import Topo
    pn, ne = 3, 4
    t = Topo(CubedSphere(pn, ne, 6), 0, 1)
    own = _owned(pn, t.all_inds1x_l(), t.all_inds1y_l())
    assert np.unique(own).size == own.size
    D = t.nDofsX
    assert own.size == 2 * D * D and t.n1 - own.size == 2 * D      # the D x-edges of the east column, the D y-edges of the north row


def test_header_declares_owned_entries():
    from mimsem_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "mimsem_hip.h")).read()
    for name, args in (("mimsem_owned_blocks_build", 9), ("mimsem_owned_blocks_apply", 9), ("mimsem_owned_block_chebyshev_solve", 18),
                       ("mimsem_ksp_set_pc_bjacobi_owned", 1)):
        m = re.search(r"int\s+%s\s*\(([^;]*)\);" % name, hdr)
        assert m, name
        assert len(m.group(1).split(",")) == args, name
        assert len(_lib._SIGS[name][1]) == args, name
