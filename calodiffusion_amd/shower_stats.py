"""The arithmetic behind the reference's plot program (calodiffusion/plot.py, the classes of calodiffusion/utils/plots.py) on the
device: the per-layer, per-radius and per-angle statistics a physicist looks at first after ``generate()``, from ONE pass over
the showers (``cd_shower_stats_compute``, include/calodiff.h "shower statistics").  The reference reshapes and sums the whole
shower set again in every class, with float temporaries the size of the set.

Only raw sums leave the device -- per shower and layer ``sum e``, ``max e``, ``sum e r``, ``sum e r^2``, ``sum e cos``, ``sum e
sin``, the cells above the hit threshold and above the sparsity epsilon, and per shower the energy in each radial and angular
bin.  The reference's rules (``np.ma.divide(...).filled(0)``, ``layer_zero = layerE < 1e-6 totalE``, ``clip(R, 1e-8, 1)``,
``sqrt(-log R)``, ``ma.sqrt(...).filled(0)``, ``std / mean``) are written once here in NumPy, on (N, L) arrays, in the methods
of ``ShowerStats`` named after the plot classes; each returns exactly the array(s) its class hands to ``_plot`` / ``_hist`` for
one sample.  Drawing, HDF5 and the command line are out of scope.

The geometry is four tables of L x n entries (n the cells of a layer), so one kernel serves the regular (N, 1, L, A, R) grid of
Dataset 2 / 3 and HGCal's (N, L, cells):

  ``ShowerStatistics.for_grid(shape_final, r_projection="reference")``
      ``angle`` = the midpoints of ``linspace(-pi, pi, A + 1)`` and ``a_bin`` = the alpha index of a cell, ``r_bin`` = its r index
      (what ``AverageER`` sums, and geometrically right).  THE REFERENCE'S QUIRK: ``AverageShowerWidth`` (plots.py:507-510)
      reshapes a layer's (A, R) cells to (R, -1) WITHOUT a transpose, so its "r bin k" is the flat cells k A ... (k + 1) A - 1 and
      not the cells of radius k.  The default reproduces that: ``r_coord = cell // A + 0.5``.  ``r_projection="radial"`` gives
      the geometric ``r_coord = cell % R + 0.5``.  The quirk is table content, not code.
  ``ShowerStatistics.for_hgcal(geom)``
      ``r_bin = ring_map`` with ``max(nrings)`` bins, ``r_coord = sqrt(xmap^2 + ymap^2)``, ``angle = theta_map``, no ``a_bin``.

Differences to the reference, all deliberate: showers are cast to float32 (as at every entry point of this package) and every sum
is fp64 where the reference sums float32 arrays in float32, so results agree with it to float32 rounding.
There is no host fallback: without a GPU or the built library ``compute`` raises.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from .abi import CdShowerStatsDesc, Handle, _check, _dev32, _ptr, _stream, load_library, require_gpu

# columns of a cd_shower_stats_compute record and of its counts
E, MAX, ER, ERR, ECOS, ESIN = range(6)
HITS, OCCUPIED = range(2)
MAX_CELLS, MAX_LAYERS, MAX_BINS = 4096, 512, 256


def grid_tables(shape_final, r_projection="reference"):
    """(r_bin, a_bin, r_coord, angle), each (L, A * R), of a regular grid SHAPE_FINAL = (..., L, A, R): see the module docstring."""
    if r_projection not in ("reference", "radial"):
        raise ValueError(f"ShowerStatistics.for_grid: r_projection must be 'reference' or 'radial', got {r_projection!r}")
    if len(shape_final) < 3:
        raise ValueError(f"ShowerStatistics.for_grid: shape_final must end in (layers, alpha bins, r bins), got {tuple(shape_final)}")
    L, A, R = (int(v) for v in shape_final[-3:])
    cell = np.arange(A * R)
    edges = np.linspace(-math.pi, math.pi, A + 1)
    mid = np.array([(edges[i] + edges[i + 1]) / 2.0 for i in range(A)])  # GetMatrix of AverageShowerWidth (plots.py:463-471)
    r_coord = (cell // A if r_projection == "reference" else cell % R) + 0.5
    rep = lambda a, dt: np.ascontiguousarray(np.broadcast_to(a, (L, A * R)), dtype=dt)  # noqa: E731
    return rep(cell % R, np.int32), rep(cell // R, np.int32), rep(r_coord, np.float64), rep(mid[cell // R], np.float64)


def hgcal_tables(geom):
    """(r_bin, None, r_coord, angle), each (L, max_ncell), of an HGCal geometry object (``ring_map``, ``xmap``, ``ymap``, ``nrings``,
    ``max_ncell`` and ``theta_map``, or none and it is ``arctan2(xmap, ymap) mod 2 pi`` as HGCal_utils.load_geom makes it)."""
    n = int(geom.max_ncell)
    x, y = np.asarray(geom.xmap, dtype=np.float64)[:, :n], np.asarray(geom.ymap, dtype=np.float64)[:, :n]
    theta = np.asarray(geom.theta_map, dtype=np.float64)[:, :n] if hasattr(geom, "theta_map") else np.arctan2(x, y) % (2.0 * np.pi)
    ring = np.asarray(geom.ring_map)[:, :n]
    if not np.array_equal(ring, np.round(ring)):
        raise ValueError("ShowerStatistics.for_hgcal: ring_map holds values that are not whole numbers")
    c = np.ascontiguousarray
    return c(ring, dtype=np.int32), None, c((x ** 2 + y ** 2) ** 0.5), c(theta)


def check_tables(who, r_bin, n_rbins, a_bin, n_abins, r_coord, angle):
    """The limits of cd_shower_stats_create, by name, before anything touches the device."""
    if r_bin.ndim != 2 or any(t is not None and t.shape != r_bin.shape for t in (a_bin, r_coord, angle)):
        raise ValueError(f"{who}: the tables must share one (layers, cells) shape")
    L, n = r_bin.shape
    if not 1 <= n <= MAX_CELLS:
        raise ValueError(f"{who}: {n} cells a layer; the device kernel stages a layer in LDS: 1 to {MAX_CELLS}")
    if not 1 <= L <= MAX_LAYERS:
        raise ValueError(f"{who}: {L} layers; 1 to {MAX_LAYERS}")
    if not 1 <= n_rbins <= MAX_BINS:
        raise ValueError(f"{who}: {n_rbins} radial bins; 1 to {MAX_BINS}")
    if not 0 <= n_abins <= MAX_BINS or (a_bin is None) != (n_abins == 0):
        raise ValueError(f"{who}: {n_abins} angular bins {'without' if a_bin is None else 'with'} an a_bin table; 1 to {MAX_BINS} with "
                         "one, 0 without")
    if r_bin.min() < -1 or r_bin.max() >= n_rbins:
        raise ValueError(f"{who}: r_bin holds indices outside [-1, {n_rbins})")
    if a_bin is not None and (a_bin.min() < -1 or a_bin.max() >= n_abins):
        raise ValueError(f"{who}: a_bin holds indices outside [-1, {n_abins})")
    if not (np.isfinite(r_coord).all() and np.isfinite(angle).all()):
        raise ValueError(f"{who}: r_coord and angle must be finite")


def _filled_divide(a, b):
    return np.ma.divide(a, b).filled(0)


class ShowerStats:
    """The raw sums of N showers (``records`` (N, L, 6) float64, ``counts`` (N, L, 2) int32, ``r_profile`` (N, n_rbins) and
    ``a_profile`` (N, n_abins) float64 or None) and what the reference's plot classes derive from them."""

    def __init__(self, records, counts, r_profile, a_profile, n_cells):
        self.records, self.counts, self.r_profile, self.a_profile, self.n_cells = records, counts, r_profile, a_profile, int(n_cells)

    # -- shared pieces ---------------------------------------------------------------------------------------------------
    @property
    def layer_energy(self):
        return self.records[:, :, E]

    def e_tot(self):
        """HistEtot (plots.py:884-887): the deposited energy of each shower, (N,): the layer energies in layer order."""
        tot = np.zeros(self.records.shape[0], dtype=np.float64)
        for l in range(self.records.shape[1]):
            tot += self.records[:, l, E]
        return tot

    def _layer_zero(self):
        return self.layer_energy < 1e-6 * self.e_tot()[:, None]

    def _angular(self):
        """ang_center_spread (plots.py:24-38) per shower and layer."""
        layer = self.layer_energy
        cos_ec, sin_ec = _filled_divide(self.records[:, :, ECOS], layer), _filled_divide(self.records[:, :, ESIN], layer)
        mean = np.arctan2(sin_ec, cos_ec)
        R = np.clip(np.sqrt(sin_ec ** 2 + cos_ec ** 2), 1e-8, 1.0)
        return mean, np.sqrt(-np.log(R))

    def _radial(self):
        """centre and width of r per shower and layer, zero in the layers below 1e-6 of the shower (GetCenter / GetWidth,
        plots.py:481-491, 41-43; RCenterHGCal :762-777)."""
        layer, zero = self.layer_energy, self._layer_zero()
        c, c2 = _filled_divide(self.records[:, :, ER], layer), _filled_divide(self.records[:, :, ERR], layer)
        c[zero] = 0.0
        c2[zero] = 0.0
        return c, np.ma.sqrt(c2 - c ** 2).filled(0)

    # -- the plot classes ------------------------------------------------------------------------------------------------
    def e_layer(self):
        """ELayer (plots.py:567-576): mean layer energy (L,), its std / mean (L,) and ``layer > 1e-6 total`` (N, L) bool."""
        layer = self.layer_energy
        mean = np.mean(layer, 0)
        with np.errstate(invalid="ignore", divide="ignore"):
            std = np.std(layer, 0) / mean
        return mean, std, layer > 1e-6 * self.e_tot()[:, None]

    def sparsity_layer(self):
        """SparsityLayer (plots.py:684-692): mean and std over the showers of the share of a layer's cells above the epsilon."""
        share = self.counts[:, :, OCCUPIED] / self.n_cells
        return np.mean(share, axis=0), np.std(share, axis=0)

    def shower_width(self):
        """AverageShowerWidth (plots.py:461-518): r centre, r width, angular centre, angular width, each (N, L).  The r
        coordinate is the geometry's ``r_coord`` (``for_grid``: the reference's reshape quirk by default); the angular pair is
        NOT zeroed in negligible layers, as in the reference."""
        rc, rw = self._radial()
        pc, pw = self._angular()
        return rc, rw, pc, pw

    def energy_r(self):
        """AverageER (plots.py:617-625): energy per r bin, (N, R)."""
        return self._need(self.r_profile, "r_profile")

    def energy_phi(self):
        """AverageEPhi (plots.py:651-658): energy per alpha bin, (N, A)."""
        return self._need(self.a_profile, "a_profile")

    def e_ratio(self, energies, norm=None):
        """HistERatio (plots.py:406-418): deposited over incident energy, divided by ``norm`` -- the mean of the Geant4 sample's
        ratio (``reference.e_ratio(energies).mean()`` with norm=1); None: this sample's own mean."""
        energies = np.asarray(energies, dtype=np.float64).reshape(-1)
        if energies.shape[0] != self.records.shape[0]:
            raise ValueError(f"e_ratio: {energies.shape[0]} energies for {self.records.shape[0]} showers")
        ratio = self.e_tot() / energies
        return ratio / (np.mean(ratio) if norm is None else norm)

    def n_hits(self):
        """HistNhits (plots.py:912-916): cells above the hit threshold per shower, (N,)."""
        return self.counts[:, :, HITS].sum(axis=1, dtype=np.int64)

    def max_e(self):
        """HistMaxE (plots.py:1003-1010): brightest cell over deposited energy per shower, (N,)."""
        return _filled_divide(self.records[:, :, MAX].max(axis=1), self.e_tot())

    def max_e_layer(self):
        """HistMaxELayer (plots.py:978-984): brightest cell of a layer over the layer's energy, (N, L)."""
        return _filled_divide(self.records[:, :, MAX], self.layer_energy)

    def radial_energy_hgcal(self):
        """RadialEnergyHGCal (plots.py:720-734): energy per ring, (N, max(nrings))."""
        return self._need(self.r_profile, "r_profile")

    def r_center_hgcal(self):
        """RCenterHGCal (plots.py:748-779): the r centres flat (N L,), their mean per layer (L,), the r widths flat and their
        mean per layer."""
        c, w = self._radial()
        return np.reshape(c, (-1)), np.mean(c, axis=0), np.reshape(w, (-1)), np.mean(w, axis=0)

    def phi_center_hgcal(self):
        """PhiCenterHGCal (plots.py:810-839): as ``r_center_hgcal`` for the angle; here negligible layers ARE zeroed."""
        c, w = self._angular()
        zero = self._layer_zero()
        c[zero] = 0.0
        w[zero] = 0.0
        return np.reshape(c, (-1)), np.mean(c, axis=0), np.reshape(w, (-1)), np.mean(w, axis=0)

    @staticmethod
    def _need(a, name):
        if a is None:
            raise ValueError(f"ShowerStats: {name} was not computed for this geometry")
        return a


class ShowerStatistics:
    """One shower geometry on the device: see the module docstring.  ``compute`` returns a ``ShowerStats``."""

    def __init__(self, r_bin, n_rbins, a_bin, n_abins, r_coord, angle, who="ShowerStatistics"):
        r_bin = np.ascontiguousarray(r_bin, dtype=np.int32)
        a_bin = None if a_bin is None else np.ascontiguousarray(a_bin, dtype=np.int32)
        r_coord, angle = np.ascontiguousarray(r_coord, dtype=np.float64), np.ascontiguousarray(angle, dtype=np.float64)
        check_tables(who, r_bin, int(n_rbins), a_bin, int(n_abins), r_coord, angle)
        self.r_bin, self.a_bin, self.r_coord, self.angle = r_bin, a_bin, r_coord, angle
        self.n_rbins, self.n_abins = int(n_rbins), int(n_abins)
        self.n_layers, self.n_cells = r_bin.shape
        self._handles = {}  # device index -> abi.Handle of a CdShowerStats
        self._lib = None

    @classmethod
    def for_grid(cls, shape_final, r_projection="reference"):
        r_bin, a_bin, r_coord, angle = grid_tables(shape_final, r_projection)
        A, R = int(shape_final[-2]), int(shape_final[-1])
        return cls(r_bin, R, a_bin, A, r_coord, angle, who="ShowerStatistics.for_grid")

    @classmethod
    def for_hgcal(cls, geom):
        r_bin, a_bin, r_coord, angle = hgcal_tables(geom)
        return cls(r_bin, int(np.max(geom.nrings)), a_bin, 0, r_coord, angle, who="ShowerStatistics.for_hgcal")

    @property
    def voxels(self):
        return self.n_layers * self.n_cells

    def _device_handle(self):
        """The handle of the current device, created on first use there."""
        device = torch.cuda.current_device() if torch.cuda.is_available() else -1
        if device not in self._handles:
            lib = load_library()
            require_gpu()
            i32 = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32))  # noqa: E731
            f64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
            desc = CdShowerStatsDesc(C.sizeof(CdShowerStatsDesc), self.n_layers, self.n_cells, self.n_rbins, self.n_abins,
                                     i32(self.r_bin), i32(self.a_bin), f64(self.r_coord), f64(self.angle))
            owner = Handle(lib.cd_shower_stats_destroy)
            _check(lib.cd_shower_stats_create(C.byref(desc), C.byref(owner.handle), _stream()))
            self._lib, self._handles[device] = lib, owner
        return self._handles[device].handle

    def close(self):
        """Frees the device tables (they are created again on the next call; an instance that goes frees them by itself)."""
        handles, self._handles = self._handles, {}
        for owner in handles.values():
            owner.close()

    def _launch(self, showers, hit_threshold, sparsity_eps, profiles=True, out=None):
        """(B, L n) fp32 device tensor -> (records, counts, r_profile, a_profile) tensors on its device (allocated here unless
        ``out`` passes them in), one cd_shower_stats_compute launch on that device's current stream."""
        B, dev = showers.shape[0], showers.device
        with torch.cuda.device(dev):
            handle = self._device_handle()
            if out is None:
                out = (torch.empty((B, self.n_layers, 6), dtype=torch.float64, device=dev),
                       torch.empty((B, self.n_layers, 2), dtype=torch.int32, device=dev),
                       torch.empty((B, self.n_rbins), dtype=torch.float64, device=dev) if profiles else None,
                       torch.empty((B, self.n_abins), dtype=torch.float64, device=dev) if profiles and self.n_abins else None)
            _check(self._lib.cd_shower_stats_compute(handle, showers.data_ptr(), B, float(hit_threshold), float(sparsity_eps),
                                                     out[0].data_ptr(), out[1].data_ptr(), _ptr(out[2]), _ptr(out[3]),
                                                     _stream()))
        return out

    def compute(self, data, hit_threshold=1e-3, sparsity_eps=1e-6, chunk=16384):
        """The statistics of ``data``: N showers of any shape with L x n elements each ((N, 1, L, A, R), (N, L, cells), flat): a
        NumPy array (or host tensor), uploaded and processed ``chunk`` showers at a time, or a CUDA tensor, used in place.
        Either is cast to float32 first.  A cell is a hit when it is ``> hit_threshold`` (HistNhits: 1 MeV) and occupied when
        it is ``> sparsity_eps`` (SparsityLayer), compared in float32."""
        shape = tuple(data.shape)
        if len(shape) < 2 or int(np.prod(shape[1:])) != self.voxels:
            raise ValueError(f"ShowerStatistics.compute: expected showers of {self.n_layers} x {self.n_cells} = {self.voxels} elements "
                             f"each, got shape {shape}")
        if int(chunk) <= 0:
            raise ValueError(f"ShowerStatistics.compute: chunk must be positive, got {chunk}")
        N, L = shape[0], self.n_layers
        rec, cnt = np.empty((N, L, 6), dtype=np.float64), np.empty((N, L, 2), dtype=np.int32)
        rp = np.empty((N, self.n_rbins), dtype=np.float64)
        ap = np.empty((N, self.n_abins), dtype=np.float64) if self.n_abins else None

        def run(part, lo):
            o = self._launch(part, hit_threshold, sparsity_eps)
            hi = lo + part.shape[0]
            rec[lo:hi], cnt[lo:hi], rp[lo:hi] = o[0].cpu().numpy(), o[1].cpu().numpy(), o[2].cpu().numpy()
            if ap is not None:
                ap[lo:hi] = o[3].cpu().numpy()

        if N:
            if isinstance(data, torch.Tensor) and data.is_cuda:
                run(_dev32(data.detach(), "data").reshape(N, self.voxels), 0)
            else:
                self._device_handle()  # (raises here without a GPU, before any upload)
                host = (data.detach().numpy() if isinstance(data, torch.Tensor) else np.asarray(data)).reshape(N, self.voxels)
                for lo in range(0, N, int(chunk)):
                    part = np.ascontiguousarray(host[lo:lo + int(chunk)], dtype=np.float32)
                    run(torch.from_numpy(part if part.flags.writeable else part.copy()).cuda(), lo)
        return ShowerStats(rec, cnt, rp, ap, self.n_cells)


# ---- histograms: the reference's binnings, counted on the device ---------------------------------------------------------------

def voxel_sample(data, n_showers=1000):
    """HistVoxelE's sample (plots.py:946-948): the cells of the first ``n_showers`` showers, flat."""
    n = min(int(n_showers), data.shape[0])
    return data[:n].reshape(-1)


def voxel_histogram(data, edges, n_showers=1000):
    """``np.histogram(voxel_sample(data, n_showers), bins=edges)[0]`` on the device (``evaluate.column_histograms``), int64."""
    from .evaluate import column_histograms
    return column_histograms(voxel_sample(data, n_showers).reshape(-1, 1), np.asarray(edges, dtype=np.float64).reshape(1, -1))[0, 0]


def _extreme(a, fn):
    return float(fn(a).item() if isinstance(a, torch.Tensor) else fn(a))


def binnings(reference_stats, generated_stats, reference_data=None, generated_data=None, n_showers=1000):
    """The bin edges the reference's histogram classes build, all from the Geant4 sample (``reference_stats``) except where the
    class looks at both: ERatio ``linspace(0.7, 1.3, 30)`` (plots.py:421), TotalE ``geomspace(1 % quantile of the positive
    energies, maximum, 20)`` (:894-898), Nhits ``linspace(min of Geant4, max of both, 20)`` (:924), MaxEnergy ``linspace(0, 1,
    10)`` (:1016) and, where both shower arrays are given, VoxelE ``geomspace(smallest positive Geant4 cell, largest cell of
    both, 50)`` over the first ``n_showers`` showers (:946-960)."""
    ref_tot = reference_stats.e_tot()
    ref_hits, gen_hits = reference_stats.n_hits(), generated_stats.n_hits()
    out = {"ERatio": np.linspace(0.7, 1.3, 30),
           "TotalE": np.geomspace(np.quantile(ref_tot[ref_tot > 0.0], 0.01), np.quantile(ref_tot, 1.0), 20),
           "Nhits": np.linspace(np.min(ref_hits), max(np.max(ref_hits), np.max(gen_hits), 0.0), 20),
           "MaxEnergy": np.linspace(0, 1, 10)}
    if reference_data is not None and generated_data is not None:
        ref, gen = voxel_sample(reference_data, n_showers), voxel_sample(generated_data, n_showers)
        v_max = max(_extreme(ref, lambda a: a.max()), _extreme(gen, lambda a: a.max()), 0.0)
        out["VoxelE"] = np.geomspace(_extreme(ref, lambda a: a[a > 0].min()), v_max, 50)
    return out


def compare(reference_stats, generated_stats, reference_energies, generated_energies, reference_data=None, generated_data=None,
            n_showers=1000):
    """The histogram classes of the plot program for a Geant4 and a generated sample: {name: {"edges", "reference", "generated"
    (int64 counts, as ``np.histogram``), "separation" (the reference's separation power of the two)}} for ERatio, TotalE, Nhits,
    MaxEnergy and (with both shower arrays) VoxelE, counted by ``evaluate.column_histograms``."""
    from .evaluate import column_histograms, separation_from_counts
    edges = binnings(reference_stats, generated_stats, reference_data, generated_data, n_showers)
    norm = np.mean(reference_stats.e_ratio(reference_energies, norm=1.0))
    values = {"ERatio": (reference_stats.e_ratio(reference_energies, norm), generated_stats.e_ratio(generated_energies, norm)),
              "TotalE": (reference_stats.e_tot(), generated_stats.e_tot()),
              "Nhits": (reference_stats.n_hits(), generated_stats.n_hits()),
              "MaxEnergy": (reference_stats.max_e(), generated_stats.max_e())}
    out = {}
    for name, (ref, gen) in values.items():
        e = edges[name].reshape(1, -1)
        x = np.concatenate([ref, gen]).astype(np.float64).reshape(-1, 1)
        counts = column_histograms(x, e, [(0, len(ref)), (len(ref), len(gen))])
        out[name] = {"edges": edges[name], "reference": counts[0, 0], "generated": counts[1, 0],
                     "separation": float(separation_from_counts(counts[0], counts[1], e)[0])}
    if "VoxelE" in edges:
        ref, gen = voxel_histogram(reference_data, edges["VoxelE"], n_showers), voxel_histogram(generated_data, edges["VoxelE"], n_showers)
        out["VoxelE"] = {"edges": edges["VoxelE"], "reference": ref, "generated": gen,
                         "separation": float(separation_from_counts(ref[None], gen[None], edges["VoxelE"][None])[0])}
    return out
