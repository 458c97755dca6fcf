"""Zonal-mean statistics of a 3-D state, accumulated on the device: what a Held-Suarez run (eul/HeldSuarez.cpp) produces.  The reference
dumps ASCII fields every 1 440 steps and averages them offline (scr/WriteFields.py, *_zonal_avg.png); here every step can be a sample:
Engine.zonal_moments (mimsem_euler_zonal_moments, csrc/zonal_stats.inc) adds the nine band sums of

    a {1, u, v, T, uu, vv, uv, vT, TT},   a = Q_q det[e][q]

of the fields Euler.quad_fields writes -- (u, v) = interp1_g(velx_k) / thick_k, T = Theta Pi / (CP r) from interp2_g(rt_k, exner_k, rho_k) /
thick_k -- to a device array [9, nk, nb] in one launch, with no read-back.  Levels are the model's geometric layers.

The band rule, stated once: the nb bands are equal in latitude, edges = linspace(-pi/2, pi/2, nb + 1), and a point of latitude phi belongs
to band searchsorted(edges[1:-1], phi, side="right"): band i holds edges[i] <= phi < edges[i+1], the last band also phi = +pi/2.  Only
the nb - 1 inner edges are searched, so a pole -- or a latitude that rounding has pushed past +-pi/2 -- falls into the first or the last
band and no index leaves [0, nb).  A point shared by several elements is counted by each of them with that element's own weight: the
sums are the element-wise quadrature of the band integrals, there is no last-writer rule.

No shift about a reference value: T is about 250 K and the eddy variance T'^2 10 .. 40 K^2, so <TT> - <T>^2 cancels four of the sixteen
digits of a double and twelve remain; the same holds with more room for the velocity moments.  A shift would make the sums depend on a
constant that save / load would have to carry.

FUSED: the kernel (True) or `composed` -- Engine.interp_quad and torch index sums, the A/B partner and second comparator, whose
index_add_ is not deterministic.  Rule of scripts/prof_zonal_stats.py: True when the kernel's median is not above the composed route's
(profiles/zonal_stats.txt)."""
import numpy as np
import torch

MOMENTS = ("1", "u", "v", "T", "uu", "vv", "uv", "vT", "TT")
CP = 1004.5                    # eul/Euler_2.cpp:29


def band_edges(nbands):
    return np.linspace(-0.5 * np.pi, 0.5 * np.pi, nbands + 1)


def band_index(lat, nbands):
    """the band rule of the module docstring: lat (any shape, radians) -> int32 indices in [0, nbands)"""
    return np.searchsorted(band_edges(nbands)[1:-1], np.asarray(lat, dtype=np.float64), side="right").astype(np.int32)


class ZonalStats:
    FUSED = True

    def __init__(self, eng, lat, nbands):
        """eng: Engine (one context); lat [nEl, mp12]: latitude of every element's quadrature points (the array Euler takes as hs_lat),
        a tensor or an array; nbands >= 1.  Builds the engine's band plan (Engine.zonal_plan): one ZonalStats per engine at a time"""
        if hasattr(eng, "halo"):
            raise NotImplementedError("ZonalStats: sharded engines are not supported")
        if int(nbands) < 1:
            raise ValueError("ZonalStats: at least one band, got %r" % (nbands,))
        lat = lat.detach().cpu().numpy() if torch.is_tensor(lat) else np.asarray(lat, dtype=np.float64)
        if lat.shape != (eng.nEl, eng.mp12):
            raise ValueError("ZonalStats: lat [nEl=%d, mp12=%d] expected, got %s" % (eng.nEl, eng.mp12, lat.shape))
        self.eng, self.nbands, self.nk = eng, int(nbands), eng.nk
        self.edges = band_edges(self.nbands)
        self.band = band_index(lat, self.nbands)
        eng.zonal_plan(self.band, self.nbands)
        self.acc = eng.zeros(len(MOMENTS), self.nk, self.nbands)
        self.count = 0
        self._flat = self._keep = self._weight = self._tI = None     # composed()'s tables, made on its first call

    # ---- sampling -----------------------------------------------------------------------------------------------------------------------
    def sample(self, state, hook_state=None):
        """one sample of state = (velx, velz, rho, rt, exner) (Euler's layouts; velz is not read).  Also the on_state hook of Euler.run as
        it is: called as sample(step, state) the first argument is the step number and is not used"""
        if hook_state is not None:
            state = hook_state
        velx, _, rho, rt, exner = state
        if self.FUSED:
            self.eng.zonal_moments(velx, rho, rt, exner, self.acc)
        else:
            self.acc += self.composed(state)
        self.count += 1

    def composed(self, state, absolute=False):
        """the same sample [9, nk, nb] from Engine.interp_quad, the thickness and torch index sums: four interpolation launches, the
        [nk, nEl, mp12] intermediates and torch's element-wise kernels.  index_add_ sums with atomics: not deterministic, never the default.
        absolute: the sums of the absolute values of the terms instead, the scale an error of a signed sum is measured against"""
        eng = self.eng
        velx, _, rho, rt, exner = state
        if self._flat is None:
            from .geom import gll_weights
            w = gll_weights(eng.mesh.m)
            Q = (w[:, None] * w[None, :]).reshape(-1)                                    # Q_q = w_qx w_qy, q = qy mp1 + qx
            self._weight = eng.tensor(Q[None, :] * np.asarray(eng.mesh.det))             # a = Q det  [nEl, mp12]
            self._tI = eng.tensor(np.asarray(eng.mesh.thickInv))                         # [nk, nEl, mp12]
            keep = np.flatnonzero(self.band.reshape(-1) >= 0)
            self._keep = torch.as_tensor(keep, device=eng.device)
            self._flat = torch.as_tensor(self.band.reshape(-1)[keep].astype(np.int64), device=eng.device)
        nlev = velx.shape[0]
        tI = self._tI[:nlev]
        uq = eng.interp_quad(1, velx) * tI[..., None]
        u, v = uq[..., 0], uq[..., 1]
        r, H, P = (eng.interp_quad(2, a) * tI for a in (rho, rt, exner))
        T = torch.where(r > 0, H * P / (CP * r), torch.full_like(r, float("nan")))
        a = self._weight.expand(nlev, -1, -1)
        terms = torch.stack([a, a * u, a * v, a * T, a * (u * u), a * (v * v), a * (u * v), a * (v * T), a * (T * T)])
        if absolute:
            terms = terms.abs()
        out = eng.zeros(len(MOMENTS), nlev, self.nbands)
        out.index_add_(2, self._flat, terms.reshape(len(MOMENTS), nlev, -1)[:, :, self._keep])
        return out

    # ---- results ------------------------------------------------------------------------------------------------------------------------
    def moments(self):
        """the raw sums [9, nk, nb] on the host (one read-back)"""
        return self.acc.detach().cpu().numpy()

    def means(self):
        """{name: [nk, nb]} from acc[m] / acc[0]: the zonal means T, u, v, the eddy covariances uv = <uv> - <u><v>, vT = <vT> - <v><T>,
        TT = <TT> - <T>^2, eke = 1/2 (<uu> - <u>^2 + <vv> - <v>^2), and lat [nb] (band centres), area [nk, nb] (acc[0] / count: the
        quadrature weight of the band).  Bands that hold no point read NaN"""
        return self.means_of(self.moments(), self.edges, self.count)

    @staticmethod
    def means_of(m, edges, count=1):
        """means() of raw sums m [9, nk, nb] with the band edges [nb + 1]"""
        with np.errstate(invalid="ignore", divide="ignore"):
            one = np.where(m[0] == 0.0, np.nan, m[0])
            u, v, T, uu, vv, uv, vT, TT = (m[i] / one for i in range(1, 9))
        return dict(T=T, u=u, v=v, uv=uv - u * v, vT=vT - v * T, TT=TT - T * T, eke=0.5 * (uu - u * u + vv - v * v),
                    lat=0.5 * (edges[:-1] + edges[1:]), area=m[0] / max(count, 1))

    def reset(self):
        self.acc.zero_()
        self.count = 0

    def save(self, path):
        """an .npz with acc, count, nbands and the band edges: what load needs to continue the sums"""
        with open(path, "wb") as f:
            np.savez(f, acc=self.moments(), count=np.int64(self.count), nbands=np.int64(self.nbands), edges=self.edges)

    def load(self, path):
        """continue the sums of a save() with the same bands and level count"""
        with np.load(path) as z:
            acc, count, nbands, edges = z["acc"], int(z["count"]), int(z["nbands"]), z["edges"]
        if nbands != self.nbands or acc.shape != tuple(self.acc.shape) or not np.array_equal(edges, self.edges):
            raise ValueError("ZonalStats.load: %s holds %d bands and sums %s, this object %d bands and %s"
                             % (path, nbands, acc.shape, self.nbands, tuple(self.acc.shape)))
        self.acc.copy_(self.eng.tensor(acc))
        self.count = count
