"""Progressive rendering over librtp's resumable render (include/rtp.h
rtp_render_resume_device): a canvas whose per-pixel render state stays on the
device and grows by passes, a per-pixel noise estimate from the running second
moment of the samples' luminance, and adaptive passes over pixel lists.

A state resumed in passes equals one render of the total sample count bit for
bit, so a pixel with ``count`` samples holds exactly what
``Device.render_pixels(spp=count)`` gives for it, however the samples were cut
into passes and whichever pixels shared them.

The estimate and the selection rule are pure functions over arrays
(noise_from_state, select_active): they need no device.
"""
from __future__ import annotations

import math

import numpy as np

from .mapper import Camera, Device, ErrorBadValue

LUMA = (0.2126, 0.7152, 0.0722)  # the weights of m2's luminance (include/rtp.h rtp_render_state)
CHECKPOINT_VERSION = 1
# ProgressiveRender.denoised's defaults (include/rtp.h rtp_denoise_params; rtp/rendering.hpp has the same)
DENOISE_LEVELS, DENOISE_SIGMA_L, DENOISE_SIGMA_A, DENOISE_NORMAL_LOG2 = 5, 4.0, 0.1, 5


def default_sigma_z(camera: Camera, ny: int) -> float:
    """The default depth tolerance per pixel of step: the camera's distance to
    its look-at point spread over the canvas rows, |look_at - position| / ny
    (computed in double from the float camera, rounded to float32; 1 for a
    camera that looks at its own position).  It needs no look at the frame."""
    c = camera.to_c()
    d = [float(c.look_at[i]) - float(c.position[i]) for i in range(3)]
    dist = math.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
    return float(np.float32(dist / ny)) if dist > 0 else 1.0


def split_passes(samplecount: int, passes: int) -> list:
    """samplecount cut into ``passes`` pass sizes as equal as possible, the
    earlier passes taking the remainder (10 in 3: 4, 3, 3), as rtp_path
    -passes does."""
    samplecount, passes = int(samplecount), int(passes)
    if passes < 1:
        raise ErrorBadValue("split_passes: passes must be >= 1")
    if samplecount < 0:
        raise ErrorBadValue("split_passes: samplecount must be >= 0")
    q, r = divmod(samplecount, passes)
    return [q + (1 if i < r else 0) for i in range(passes)]


def state_finite(sums: np.ndarray, m2: np.ndarray) -> np.ndarray:
    """Per pixel: its rgb sums and m2 are all finite (a NaN sample poisons both)."""
    sums = np.asarray(sums)
    return np.isfinite(sums[:, :3]).all(axis=1) & np.isfinite(np.asarray(m2))


def noise_from_state(sums: np.ndarray, m2: np.ndarray, count: np.ndarray) -> np.ndarray:
    """The relative standard error of each pixel's mean luminance, float64 [N].

    With n = count, Y = luminance of the rgb sums (= the sum of the samples'
    luminances y) and m2 = the sum of y*y:  mean = Y / n, the unbiased sample
    variance s2 = (m2 - Y*Y/n) / (n - 1) (clamped at 0), and the estimate is
    sqrt(s2 / n) / mean.  A pixel whose samples all have the same luminance
    gives 0 (a black pixel too).  inf: fewer than two samples (no estimate
    yet), or a non-finite state (state_finite; never refined, see
    select_active)."""
    sums = np.asarray(sums, dtype=np.float64)
    m2 = np.asarray(m2, dtype=np.float64)
    n = np.asarray(count, dtype=np.float64)
    if sums.ndim != 2 or sums.shape[1] < 3 or m2.shape != (sums.shape[0],) or n.shape != m2.shape:
        raise ErrorBadValue("noise_from_state: expects sums [N, >=3], m2 [N] and count [N]")
    out = np.full(m2.shape, np.inf)
    ok = state_finite(sums, m2) & (n >= 2)
    Y = LUMA[0] * sums[ok, 0] + LUMA[1] * sums[ok, 1] + LUMA[2] * sums[ok, 2]
    k = n[ok]
    spread = m2[ok] - Y * Y / k
    # (the sums and m2 are float32 accumulations, each rounded per sample: a
    # spread within 1e-6 of m2 is their rounding, not variance)
    s2 = np.where(spread <= 1e-6 * m2[ok], 0.0, spread) / (k - 1)
    sem = np.sqrt(s2 / k)
    mean = Y / k
    with np.errstate(invalid="ignore", divide="ignore"):
        out[ok] = np.where(sem == 0.0, 0.0, np.where(mean > 0, sem / mean, np.inf))
    return out


def select_active(noise: np.ndarray, count: np.ndarray, spp: int, threshold: float, max_spp: int,
                  finite: np.ndarray | None = None) -> np.ndarray:
    """refine's rule: the pixels (ascending int64 ids) with noise > threshold
    whose count + spp stays within max_spp.  Pixels with a non-finite state
    (finite false; without the mask, NaN noise) are never selected: more
    samples cannot repair a NaN sum."""
    noise = np.asarray(noise, dtype=np.float64)
    count = np.asarray(count, dtype=np.int64)
    sel = (noise > float(threshold)) & (count + int(spp) <= int(max_spp))
    if finite is not None:
        sel &= np.asarray(finite, dtype=bool)
    return np.flatnonzero(sel).astype(np.int64)


def _wrap_i32(a: np.ndarray) -> np.ndarray:
    return np.asarray(a, dtype=np.uint32).view(np.int32)


class ProgressiveRender:
    """A canvas rendered in passes.  Device tensors (torch, on the device of
    ``device``): sums float32 [N, 4], seed and live int32 [N] (the library's
    uint32 words), m2 float32 [N], count int32 [N] (samples per pixel so far).
    The scene is the device's current one (set it before the first step and
    keep it)."""

    def __init__(self, device: Device, camera: Camera, nx: int, ny: int, depth: int, seed_base: int = 0):
        import torch

        if nx <= 0 or ny <= 0:
            raise ErrorBadValue("ProgressiveRender: nx and ny must be positive")
        self.device, self.camera = device, camera
        self.nx, self.ny, self.depth, self.seed_base = int(nx), int(ny), int(depth), int(seed_base) & 0xFFFFFFFF
        n = self.nx * self.ny
        self._td = torch.device("cuda", device.device)
        seeds = (np.arange(n, dtype=np.uint64) + np.uint64(self.seed_base)).astype(np.uint32)  # u32 wrap
        self.sums = torch.zeros((n, 4), dtype=torch.float32, device=self._td)
        self.seed = torch.from_numpy(_wrap_i32(seeds).copy()).to(self._td)
        self.live = torch.zeros(n, dtype=torch.int32, device=self._td)
        self.m2 = torch.zeros(n, dtype=torch.float32, device=self._td)
        self.count = torch.zeros(n, dtype=torch.int32, device=self._td)
        self._guides = None  # guides(): rendered on first use

    @property
    def n_pixels(self) -> int:
        return self.nx * self.ny

    def _stream(self) -> int:
        import torch

        return torch.cuda.current_stream(self._td).cuda_stream

    def step(self, spp: int, active=None) -> None:
        """spp more samples of every pixel, or of the pixels in ``active``
        (distinct ids): their state is gathered into compact buffers, resumed
        over the pixel list and scattered back.  Asynchronous (the torch
        current stream)."""
        import torch

        spp = int(spp)
        if spp < 0:
            raise ErrorBadValue("ProgressiveRender.step: spp must be >= 0")
        if active is None:
            self.device.render_resume_device(self.camera, self.nx, self.ny, spp, self.depth, self.sums.data_ptr(),
                                             self.seed.data_ptr(), live_ptr=self.live.data_ptr(),
                                             m2_ptr=self.m2.data_ptr(), stream=self._stream())
            self.count += spp
            return
        idx = torch.as_tensor(active, dtype=torch.int64, device=self._td).reshape(-1).contiguous()
        if idx.numel() == 0:
            return
        if int(idx.min()) < 0 or int(idx.max()) >= self.n_pixels or torch.unique(idx).numel() != idx.numel():
            raise ErrorBadValue("ProgressiveRender.step: active must hold distinct pixel ids of the canvas")
        c_sums, c_seed = self.sums[idx].contiguous(), self.seed[idx].contiguous()
        c_live, c_m2 = self.live[idx].contiguous(), self.m2[idx].contiguous()
        self.device.render_resume_device(self.camera, self.nx, self.ny, spp, self.depth, c_sums.data_ptr(),
                                         c_seed.data_ptr(), live_ptr=c_live.data_ptr(), m2_ptr=c_m2.data_ptr(),
                                         pixel_count=idx.numel(), pixel_ids_ptr=idx.data_ptr(), stream=self._stream())
        self.sums[idx], self.seed[idx], self.live[idx], self.m2[idx] = c_sums, c_seed, c_live, c_m2
        self.count[idx] += spp

    def state(self) -> dict:
        """Host copies: sums float32 [N, 4], seed / live uint32 [N], m2 float32 [N], count int32 [N]."""
        return dict(sums=self.sums.cpu().numpy(), seed=self.seed.cpu().numpy().view(np.uint32),
                    live=self.live.cpu().numpy().view(np.uint32), m2=self.m2.cpu().numpy(),
                    count=self.count.cpu().numpy())

    def image(self) -> np.ndarray:
        """Normalised colours float32 [N, 4] with NormalizeFunctor's arithmetic
        (rtp_normalize: rgb NaN -> 0, sqrt(c / count) in float) and each
        pixel's own count; for a uniform count it equals normalize()."""
        a = self.sums.cpu().numpy().copy()
        rgb = a[:, :3]
        rgb[np.isnan(rgb)] = 0
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.sqrt(a / self.count.cpu().numpy().astype(np.float32)[:, None])

    def noise(self) -> np.ndarray:
        s = self.state()
        return noise_from_state(s["sums"], s["m2"], s["count"])

    # ----------------------------------------------------------- preview --
    def guides(self) -> dict:
        """The camera's first-hit guides (Device.render_guides_device) as
        device tensors, rendered once and cached: g0 float32 [N, 4] (normal
        facing the ray, t), g1 float32 [N, 4] (texture colour, hit flag), prim
        int32 [N].  Asynchronous like step()."""
        import torch

        if self._guides is None:
            n = self.n_pixels
            g0 = torch.empty((n, 4), dtype=torch.float32, device=self._td)
            g1 = torch.empty((n, 4), dtype=torch.float32, device=self._td)
            prim = torch.empty(n, dtype=torch.int32, device=self._td)
            self.device.render_guides_device(self.camera, self.nx, self.ny, g0.data_ptr(), g1.data_ptr(),
                                             prim.data_ptr(), stream=self._stream())
            self._guides = dict(g0=g0, g1=g1, prim=prim)
        return self._guides

    def default_sigma_z(self) -> float:
        """denoised's default depth tolerance per pixel of step (default_sigma_z above)."""
        return default_sigma_z(self.camera, self.ny)

    def denoised_device(self, levels: int = DENOISE_LEVELS, sigma_l: float = DENOISE_SIGMA_L, sigma_z=None,
                        sigma_a: float = DENOISE_SIGMA_A, normal_log2: int = DENOISE_NORMAL_LOG2,
                        use_guides: bool = True):
        """The filtered linear means, a device tensor float32 [N, 4] (rgb and
        the variance of the filtered luminance mean; a pixel nothing could
        fill keeps (0, 0, 0, -1)): Device.resolve_device on the state, then
        Device.denoise_device over guides().  Nothing leaves the device and
        the state is not touched.  Defaults: 5 levels (a 125-pixel-wide
        footprint), sigma_l 4 standard deviations of the centre's mean,
        sigma_z default_sigma_z(), sigma_a 0.1 in albedo units, normal_log2 5
        (cosine to the 32nd power)."""
        import torch

        n = self.n_pixels
        g = self.guides() if use_guides else None
        if sigma_z is None:
            sigma_z = self.default_sigma_z() if use_guides else 1.0
        cv = torch.empty((n, 4), dtype=torch.float32, device=self._td)
        out, scratch = torch.empty_like(cv), torch.empty_like(cv)
        self.device.resolve_device(self.sums.data_ptr(), n, cv.data_ptr(), m2_ptr=self.m2.data_ptr(),
                                   count_ptr=self.count.data_ptr(), stream=self._stream())
        self.device.denoise_device(cv.data_ptr(), self.nx, self.ny, out.data_ptr(), scratch.data_ptr(),
                                   g0_ptr=g["g0"].data_ptr() if g else 0, g1_ptr=g["g1"].data_ptr() if g else 0,
                                   levels=levels, sigma_l=sigma_l, sigma_z=sigma_z, sigma_a=sigma_a,
                                   normal_log2=normal_log2, stream=self._stream())
        return out

    def denoised(self, **kw) -> np.ndarray:
        """denoised_device as an image, numpy float32 [N, 4]: sqrt of the rgb
        like image() (a pixel nothing could fill is black), w = the variance."""
        a = self.denoised_device(**kw).cpu().numpy()
        a[:, :3] = np.sqrt(a[:, :3])
        return a

    def refine(self, spp: int, threshold: float, max_spp: int) -> int:
        """One adaptive pass: spp more samples of the pixels select_active
        picks.  Returns their number."""
        s = self.state()
        idx = select_active(noise_from_state(s["sums"], s["m2"], s["count"]), s["count"], spp, threshold, max_spp,
                            finite=state_finite(s["sums"], s["m2"]))
        if idx.size:
            self.step(spp, active=idx)
        return int(idx.size)

    # ------------------------------------------- adaptive, on the device --
    def noise_device(self):
        """The noise estimate as a device tensor float32 [N]
        (adaptive.noise_device: include/rtp_adaptive.h states it in float32;
        noise() is the float64 host estimate).  Asynchronous like step()."""
        import torch

        from . import adaptive

        out = torch.empty(self.n_pixels, dtype=torch.float32, device=self._td)
        adaptive.noise_device(self.device, self.sums.data_ptr(), self.m2.data_ptr(), self.count.data_ptr(),
                              self.n_pixels, out.data_ptr(), stream=self._stream())
        return out

    def refine_device(self, spp: int, threshold: float, max_spp: int) -> int:
        """refine() without leaving the device (adaptive.refine_device): the
        estimate, the selection, the gather, the resume pass and the scatter
        run on the torch current stream; only the number of selected pixels
        comes back, which is returned.  The rule is refine()'s in float32."""
        from . import adaptive

        total, _ = adaptive.refine_device(self.device, self.camera, self.nx, self.ny, self.depth,
                                          self.sums.data_ptr(), self.seed.data_ptr(), self.m2.data_ptr(),
                                          self.count.data_ptr(), spp, threshold, max_spp,
                                          live_ptr=self.live.data_ptr(), stream=self._stream())
        return total

    def converge(self, spp: int, threshold: float, max_spp: int, max_passes: int) -> list:
        """refine_device passes until one selects nothing or max_passes have
        run (adaptive.render_adaptive_device): what each pass selected, a
        final 0 included."""
        from . import adaptive

        return adaptive.render_adaptive_device(self.device, self.camera, self.nx, self.ny, self.depth,
                                               self.sums.data_ptr(), self.seed.data_ptr(), self.m2.data_ptr(),
                                               self.count.data_ptr(), spp, threshold, max_spp, max_passes,
                                               live_ptr=self.live.data_ptr(), stream=self._stream())

    # -------------------------------------------------------- checkpoint --
    def save(self, path: str) -> None:
        """An .npz checkpoint: the state arrays, camera, sizes, depth, seed base."""
        cam = self.camera
        with open(path, "wb") as f:
            np.savez(f, **checkpoint_arrays(self.state(), cam, self.nx, self.ny, self.depth, self.seed_base))

    @classmethod
    def load(cls, device: Device, path: str) -> "ProgressiveRender":
        import torch

        ck = read_checkpoint(path)
        cam = Camera()
        cam.SetPosition(ck["cam_position"])
        cam.SetLookAt(ck["cam_look_at"])
        cam.SetViewUp(ck["cam_view_up"])
        cam.SetFieldOfView(ck["cam_fov"])
        r = cls(device, cam, ck["nx"], ck["ny"], ck["depth"], ck["seed_base"])
        r.sums.copy_(torch.from_numpy(ck["sums"]))
        r.seed.copy_(torch.from_numpy(_wrap_i32(ck["seed"]).copy()))
        r.live.copy_(torch.from_numpy(_wrap_i32(ck["live"]).copy()))
        r.m2.copy_(torch.from_numpy(ck["m2"]))
        r.count.copy_(torch.from_numpy(ck["count"]))
        return r


_CK_ARRAYS = (("sums", np.float32, 2), ("seed", np.uint32, 1), ("live", np.uint32, 1), ("m2", np.float32, 1),
              ("count", np.int32, 1))


def checkpoint_arrays(state: dict, cam: Camera, nx: int, ny: int, depth: int, seed_base: int) -> dict:
    """What ProgressiveRender.save writes (a dict of arrays for np.savez)."""
    d = {k: np.ascontiguousarray(state[k], dtype=dt) for k, dt, _ in _CK_ARRAYS}
    d.update(version=np.int32(CHECKPOINT_VERSION), nx=np.int32(nx), ny=np.int32(ny), depth=np.int32(depth),
             seed_base=np.uint32(seed_base), cam_position=np.asarray(cam.position, dtype=np.float32),
             cam_look_at=np.asarray(cam.look_at, dtype=np.float32),
             cam_view_up=np.asarray(cam.view_up, dtype=np.float32), cam_fov=np.float32(cam.fov))
    return d


def read_checkpoint(path: str) -> dict:
    """Read and check a checkpoint: every array must have the dtype and the
    shape the sizes in the file ask for (ErrorBadValue otherwise)."""
    with np.load(path, allow_pickle=False) as z:
        ck = {k: z[k] for k in z.files}
    need = [k for k, _, _ in _CK_ARRAYS] + ["version", "nx", "ny", "depth", "seed_base", "cam_position", "cam_look_at",
                                            "cam_view_up", "cam_fov"]
    missing = [k for k in need if k not in ck]
    if missing:
        raise ErrorBadValue(f"checkpoint {path}: missing {missing}")
    if int(ck["version"]) != CHECKPOINT_VERSION:
        raise ErrorBadValue(f"checkpoint {path}: version {int(ck['version'])}, expected {CHECKPOINT_VERSION}")
    for k in ("nx", "ny", "depth", "seed_base"):
        ck[k] = int(ck[k])
    ck["cam_fov"] = float(ck["cam_fov"])
    n = ck["nx"] * ck["ny"]
    if ck["nx"] <= 0 or ck["ny"] <= 0 or ck["depth"] < 1:
        raise ErrorBadValue(f"checkpoint {path}: bad sizes {ck['nx']} x {ck['ny']}, depth {ck['depth']}")
    for k, dt, nd in _CK_ARRAYS:
        shape = (n, 4) if nd == 2 else (n,)
        if ck[k].dtype != dt or ck[k].shape != shape:
            raise ErrorBadValue(f"checkpoint {path}: {k} is {ck[k].dtype}{ck[k].shape}, expected "
                                f"{np.dtype(dt).name}{shape} for a {ck['nx']} x {ck['ny']} canvas")
    for k in ("cam_position", "cam_look_at", "cam_view_up"):
        if ck[k].shape != (3,):
            raise ErrorBadValue(f"checkpoint {path}: {k} must have 3 components")
    if (ck["count"] < 0).any():
        raise ErrorBadValue(f"checkpoint {path}: negative sample count")
    return ck
