"""Self-supervised depth / ego-motion / object-motion loss of the sequence branch (reference model/modeling/monodepth_loss.py:397-844).

`MonodepthLoss(cfg, **flags)` has the reference's methods and dictionary keys.  What the reference expects a trainer to set from outside
(`bool_MotMask`, `bool_CmpFlow`, `bool_automask`, `move_Depth`, `move_CmpFlow`, `move_MotMask`, `step`, `phrage`) are keyword arguments
here and stay plain attributes.  Its two random draws are injectable: `tie_noise=[(B, 2, H, W)] * 4` is the `randn` of the auto-mask
tie-break (multiplied by 1e-5 as there), `ground_samples=[(B, 500) int64] * 4` the point indices of the ground-plane RANSAC; when they are
not given they are drawn on the device from the module's `torch.Generator`.

CPU tensors (or `impl="torch"`) run the reference's op sequence in plain torch.  CUDA tensors run two fused stages of csrc/monodepth.hip:

    uenc_view_synth_fwd / _bwd    disparity upsample, depth, back-projection, flows, projections and the colour sampling of every
                                  (scale, frame, image) in one launch
    uenc_photo_loss_fwd / _bwd    SSIM + L1 of every candidate, the minimum with its index, and the mean per scale

The regularisers (d_smooth, c_smooth, m_smooth, c_consistency, m_sparsity, d_ground) are torch compositions on both paths, written so that
nothing reads a value back to the host: `m_sparsity`'s `if torch.all(...)` is a 0 / 1 factor and its masked mean a sum over the mask
divided by its count; the 3x3 inverse of the plane fit is a closed-form adjugate (the fits are solved in float64); masked assignments are `torch.where`.

Two deviations, kernel path only: `("depth", 0, s)` / `("disp_scaled", 0, s)` carry no autograd history (the loss never differentiates
them), and `("cam_points", 0, s)`, `("ego_flow", f, s)`, `("independ_flow", f, s)` are not materialised.
Out of scope as in the issue: plotting, the two prints, compute_depth_errors, the stereo frame id "s".
"""
from typing import Optional, Sequence

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

__all__ = ["MonodepthLoss", "GroundPlane", "SSIM", "disp_to_depth", "depth_to_disp", "compute_smooth_loss", "interp"]

LOSS_TERMS = ["p_photo", "d_smooth", "d_ground", "c_smooth", "c_consistency", "m_sparsity", "m_smooth"]
COEFS = {"g_p_photo": 1.0, "g_d_smooth": 1e-3, "g_d_ground": 0.1, "g_c_smooth": 1e-3, "g_c_consistency": 5.0, "g_m_sparsity": 0.04,
         "g_m_smooth": 0.1}
WEIGHT_RAMP = ["g_c_smooth", "g_c_consistency", "g_m_sparsity", "g_m_smooth"]
TIE_NOISE_SCALE = 0.00001
NUM_SCALES = 4


def disp_to_depth(disp, min_depth=0.1, max_depth=100.0):
    min_disp, max_disp = 1 / max_depth, 1 / min_depth
    scaled_disp = min_disp + (max_disp - min_disp) * disp
    return scaled_disp, 1 / scaled_disp


def depth_to_disp(depth, min_depth=0.1, max_depth=100.0):
    min_disp, max_disp = 1 / max_depth, 1 / min_depth
    return (1 / depth - min_disp) / (max_disp - min_disp)


def interp(x, shape, mode="bilinear", align_corners=False):
    return F.interpolate(x, shape, mode=mode, align_corners=align_corners)


def compute_smooth_loss(inp, img=None):
    """Edge-aware first-order smoothness of (B, C, H, W) (monodepth_loss.py:293-308)."""
    gx = torch.abs(inp[:, :, :, :-1] - inp[:, :, :, 1:])
    gy = torch.abs(inp[:, :, :-1, :] - inp[:, :, 1:, :])
    if img is not None:
        gx = gx * torch.exp(-torch.mean(torch.abs(img[:, :, :, :-1] - img[:, :, :, 1:]), 1, keepdim=True))
        gy = gy * torch.exp(-torch.mean(torch.abs(img[:, :, :-1, :] - img[:, :, 1:, :]), 1, keepdim=True))
    return gx.mean() + gy.mean()


class SSIM(nn.Module):
    """(1 - SSIM) / 2 over 3x3 average pools of the reflection-padded images, clamped to [0, 1] (monodepth_loss.py:311-343)."""
    C1, C2 = 0.01 ** 2, 0.03 ** 2

    def forward(self, x, y):
        x, y = F.pad(x, (1, 1, 1, 1), mode="reflect"), F.pad(y, (1, 1, 1, 1), mode="reflect")
        mu_x, mu_y = F.avg_pool2d(x, 3, 1), F.avg_pool2d(y, 3, 1)
        sigma_x = F.avg_pool2d(x ** 2, 3, 1) - mu_x ** 2
        sigma_y = F.avg_pool2d(y ** 2, 3, 1) - mu_y ** 2
        sigma_xy = F.avg_pool2d(x * y, 3, 1) - mu_x * mu_y
        n = (2 * mu_x * mu_y + self.C1) * (2 * sigma_xy + self.C2)
        d = (mu_x ** 2 + mu_y ** 2 + self.C1) * (sigma_x + sigma_y + self.C2)
        return torch.clamp((1 - n / d) / 2, 0, 1)


def _pix_coords(h, w, device, dtype):
    """(3, h * w): x, y, 1 of every pixel, row-major."""
    ys, xs = torch.meshgrid(torch.arange(h, device=device, dtype=dtype), torch.arange(w, device=device, dtype=dtype), indexing="ij")
    return torch.stack([xs.reshape(-1), ys.reshape(-1), torch.ones(h * w, device=device, dtype=dtype)], 0)


def _backproject(depth, inv_K, pix):
    """(B, 1, h, w) depth -> homogeneous camera points (B, 4, h * w) (BackprojectDepth, monodepth_loss.py:256-261)."""
    B = depth.shape[0]
    cam = depth.reshape(B, 1, -1) * torch.matmul(inv_K[:, :3, :3], pix[None])
    return torch.cat([cam, torch.ones_like(cam[:, :1])], 1)


def _project(points, K, T, H, W, eps=1e-7):
    """Project3D (monodepth_loss.py:276-290): grid_sample coordinates (B, H, W, 2) and the ego flow (B, 3, H * W)."""
    p3 = torch.matmul(T, points) if T is not None else points
    cam = torch.matmul(K[:, :3, :], p3)
    pix = cam[:, :2, :] / (cam[:, 2, :].unsqueeze(1) + eps)
    pix = pix.reshape(-1, 2, H, W).permute(0, 2, 3, 1)
    pix = torch.stack([pix[..., 0] / (W - 1), pix[..., 1] / (H - 1)], -1)
    return (pix - 0.5) * 2, p3[:, :3] - points[:, :3]


class GroundPlane(nn.Module):
    """RANSAC fit of y = w1 x + w2 z + w3 to the lower part of a point map (monodepth_loss.py:13-100).  `samples` (B, num_points_per_it *
    max_it) int64 are the point indices the reference draws with np.random.choice."""

    def __init__(self, num_points_per_it=5, max_it=25, tol=0.1, g_prior=0.5, vertical_axis=1):
        super().__init__()
        self.num_points_per_it, self.max_it, self.tol, self.g_prior, self.vertical_axis = num_points_per_it, max_it, tol, g_prior, vertical_axis

    def num_ground_points(self, H, W):
        rows = int(self.g_prior * H)
        return (rows if rows > 0 else H) * W               # `points[:, :, -0:]` is every row

    def forward(self, points, samples):
        B, _, H, W = points.shape
        ground = points[:, :, -int(self.g_prior * H):, :].reshape(B, 3, -1).permute(0, 2, 1)
        param = self.estimate_ground_plane(ground, samples)
        every = points.reshape(B, 3, H * W).permute(0, 2, 1)
        dist = self.dist_from_plane(every, param).permute(0, 2, 1).reshape(B, 1, H, W)
        return dist.detach(), param.detach()

    def get_AB(self, points):
        v = self.vertical_axis
        Bv = points[..., v:v + 1]
        A = torch.cat([points[..., i:i + 1] for i in range(3) if i != v] + [torch.ones_like(Bv)], -1)
        return A, Bv

    def dist_from_plane(self, points, param):
        A, Bv = self.get_AB(points)
        return A @ param - Bv

    def estimate_ground_plane(self, points, samples):
        B, N, _ = points.shape
        rand_points = torch.gather(points, 1, samples.to(points.device)[:, :, None].expand(-1, -1, 3))      # (B, T, 3)
        ws = self.calc_param(rand_points).reshape(-1, 3, 1)                 # (B * max_it, 3, 1)
        ps = points.repeat(self.max_it, 1, 1)                               # (B * max_it, N, 3): row k is image k % B, as in the reference
        abs_dist = torch.abs(self.dist_from_plane(ps, ws)).reshape(B, self.max_it, N)
        best = (abs_dist < self.tol).to(points.dtype).mean(2).argmax(1)
        return torch.gather(ws.reshape(B, self.max_it, 3, 1), 1, best[:, None, None, None].expand(-1, 1, 3, 1))[:, 0]

    def calc_param(self, points):
        """Least-squares plane through each group of num_points_per_it points, by the normal equations as in the reference.  They square
        the condition number of five nearly collinear points, and fp32 products summed in another order (CPU, GPU) then move the result
        in its fourth digit: the B * max_it tiny systems are formed and solved in float64 and the parameters cast back."""
        pts = points.reshape(-1, self.num_points_per_it, 3).double()
        A, Bv = self.get_AB(pts)
        At = A.transpose(2, 1)
        w = _inverse3x3(At @ A + 1e-6) @ At @ Bv
        return w.to(points.dtype).reshape(points.size(0), self.max_it, 3, 1)


def _inverse3x3(M):
    """Inverse of (n, 3, 3) as adjugate / determinant: no pivoting, so no LAPACK call and no host read."""
    a, b, c = M[:, 0, 0], M[:, 0, 1], M[:, 0, 2]
    d, e, f = M[:, 1, 0], M[:, 1, 1], M[:, 1, 2]
    g, h, i = M[:, 2, 0], M[:, 2, 1], M[:, 2, 2]
    A, Bc, C = e * i - f * h, -(d * i - f * g), d * h - e * g
    det = a * A + b * Bc + c * C
    adj = torch.stack([A, -(b * i - c * h), b * f - c * e,
                       Bc, a * i - c * g, -(a * f - c * d),
                       C, -(a * h - b * g), a * e - b * d], -1).reshape(-1, 3, 3)
    return adj / det[:, None, None]


# ---- the two fused stages as autograd functions (GPU) ------------------------------------------------------------------------------------
class _ViewSynth(torch.autograd.Function):
    """inputs: mode, K, inv_K, src (NF, B, 3, H, W), T (NF, B, 4, 4), then 4 disp, [8 complete_flow (scale-major), [8 motion_mask]].
    outputs: color (S, NF, B, 3, H, W), 8 residual flows (B, 3, H, W) (mode >= 1), then without gradient sample, sample_ego,
    sample_complete (S, NF, B, H, W, 2) and depth (S, B, 1, H, W)."""

    @staticmethod
    def forward(ctx, mode, K, inv_K, src, T, *maps):
        from .. import kernels as Kn
        S = NUM_SCALES
        NF = src.shape[0]
        disps = list(maps[:S])
        cflows = list(maps[S:S + S * NF]) if mode >= 1 else None
        masks = list(maps[S + S * NF:S + 2 * S * NF]) if mode >= 2 else None
        out = Kn.view_synth_fwd(mode, K, inv_K, src, T, disps, cflows, masks)
        ctx.mode, ctx.n_maps = mode, len(maps)
        ctx.save_for_backward(K, inv_K, src, T, *maps)
        res = out["residual"] if mode >= 1 else []
        nd = [out["sample"], out["depth"]] + ([out["sample_ego"], out["sample_complete"]] if mode >= 1 else [])
        ctx.mark_non_differentiable(*nd)
        ctx.n_res = len(res)
        return (out["color"], *res, *nd)

    @staticmethod
    def backward(ctx, gcolor, *rest):
        from .. import kernels as Kn
        K, inv_K, src, T, *maps = ctx.saved_tensors
        S, NF, mode = NUM_SCALES, src.shape[0], ctx.mode
        gres = list(rest[:ctx.n_res]) if mode >= 1 else None
        disps = list(maps[:S])
        cflows = list(maps[S:S + S * NF]) if mode >= 1 else None
        masks = list(maps[S + S * NF:S + 2 * S * NF]) if mode >= 2 else None
        gT, gdisp, gcf, gmask = Kn.view_synth_bwd(mode, K, inv_K, src, T, disps, cflows, masks, gcolor, gres)
        grads = list(gdisp) + (list(gcf) if mode >= 1 else []) + (list(gmask) if mode >= 2 else [])
        return (None, None, None, None, gT, *grads)


class _PhotoLoss(torch.autograd.Function):
    """color (S, NF, B, 3, H, W), target (B, 3, H, W), src (NF, B, 3, H, W), noise (S, B, NF, H, W) or None -> p_photo (S,) and, without
    gradient, the index of the selected candidate (S, B, H, W) uint8 (identity frames first when auto-masking)."""

    @staticmethod
    def forward(ctx, color, target, src, noise):
        from .. import kernels as Kn
        p, arg = Kn.photo_loss_fwd(color, target, src, noise)
        ctx.save_for_backward(color, target, arg)
        ctx.automask = noise is not None
        ctx.mark_non_differentiable(arg)
        return p, arg

    @staticmethod
    def backward(ctx, gp, _garg):
        from .. import kernels as Kn
        color, target, arg = ctx.saved_tensors
        return Kn.photo_loss_bwd(color, target, arg, gp.contiguous(), ctx.automask), None, None, None


class MonodepthLoss(nn.Module):
    """cfg keys read: SOLVER.IMS_PER_BATCH // len(DATASETS.TRAIN) (images per call), INPUT.DEPTH_CROP.SIZE (H, W), MODEL.DEVICE.

    Flags (the reference leaves them to the trainer; defaults here are the plain photometric baseline):
      bool_MotMask / bool_CmpFlow / bool_automask = False    the motion mask / the complete 3-D flow are predicted; auto-masking is on
      move_Depth = True, move_CmpFlow = False, move_MotMask = False    which groups of regularisers are active
      step = 0, phrage = "pretrain"    position on the weight ramp: 3 step / 8000 in the phases "mask init" and "finetune", else 3 step / 35000
      impl = None    "torch" forces the torch composition on the GPU, "kernels" demands the fused path; None chooses by device
      seed = 0       seed of the generator behind the draws that are not injected
    """

    def __init__(self, cfg, bool_MotMask=False, bool_CmpFlow=False, bool_automask=False, move_Depth=True, move_CmpFlow=False,
                 move_MotMask=False, step=0, phrage="pretrain", impl: Optional[str] = None, seed: int = 0):
        super().__init__()
        if impl not in (None, "torch", "kernels"):
            raise ValueError(f'MonodepthLoss: impl must be "torch", "kernels" or None, got {impl!r}')
        self.batch_size = cfg.SOLVER.IMS_PER_BATCH // len(cfg.DATASETS.TRAIN)
        self.height, self.width = (int(v) for v in cfg.INPUT.DEPTH_CROP.SIZE)
        self.device = cfg.MODEL.DEVICE
        self.bool_MotMask, self.bool_CmpFlow, self.bool_automask = bool_MotMask, bool_CmpFlow, bool_automask
        self.move_Depth, self.move_CmpFlow, self.move_MotMask = move_Depth, move_CmpFlow, move_MotMask
        self.step, self.phrage = step, phrage
        self.impl, self.seed = impl, seed
        self.ssim = SSIM()
        self.gp_prior, self.gp_tol, self.gp_max_it, self.gp_num_points_per_it = 0.4, 0.005, 100, 5
        self.gplane = GroundPlane(num_points_per_it=self.gp_num_points_per_it, max_it=self.gp_max_it, tol=self.gp_tol, g_prior=self.gp_prior)
        self.mask_disp_thrd = 0.03
        self.frame_ids = [-1, 1]
        self.count = 0
        self._pix, self._gen, self._fused = {}, {}, None

    # ---- helpers ------------------------------------------------------------------------------------------------------------------------
    def pix_coords(self, scale, ref):
        H, W = self.height, self.width
        key = (scale, str(ref.device), ref.dtype)
        if key not in self._pix:
            self._pix[key] = _pix_coords(H // 2 ** scale, W // 2 ** scale, ref.device, ref.dtype)
        return self._pix[key]

    def generator(self, device):
        key = str(torch.device(device))
        if key not in self._gen:
            self._gen[key] = torch.Generator(device=device).manual_seed(self.seed)
        return self._gen[key]

    def _use_kernels(self, t):
        if self.impl == "kernels" and not t.is_cuda:
            raise ValueError('MonodepthLoss: impl="kernels" needs GPU inputs')
        return t.is_cuda and self.impl != "torch" and t.dtype == torch.float32

    def _check(self, outputs, targets):
        _, H, W = targets[0][("color", 0, 0)].shape
        if (H, W) != (self.height, self.width):
            raise ValueError(f"MonodepthLoss: images are {H} x {W}, INPUT.DEPTH_CROP.SIZE is {self.height} x {self.width}")
        for s in range(NUM_SCALES):
            B, _, h, w = outputs[("disp", 0, s)].shape
            assert h * 2 ** s == H and w * 2 ** s == W
        return B, H, W

    # ---- view synthesis -----------------------------------------------------------------------------------------------------------------
    def generate_images_pred(self, outputs, targets):
        """Writes the warped colour images and everything on the way to them into `outputs` (monodepth_loss.py:427-517)."""
        B, H, W = self._check(outputs, targets)
        self.count += 1
        disp0 = outputs[("disp", 0, 0)]
        K = torch.stack([t["K"] for t in targets])
        inv_K = torch.stack([t["inv_K"] for t in targets])
        src = [torch.stack([t[("color", f, 0)] for t in targets]) for f in self.frame_ids]
        self._fused = None
        if self._use_kernels(disp0):
            return self._generate_kernels(outputs, K, inv_K, src, B, H, W)
        pix = self.pix_coords(0, disp0)
        for scale in range(NUM_SCALES):
            disp_lr = outputs[("disp", 0, scale)]
            h, w = disp_lr.shape[-2:]
            disp_scaled, depth = disp_to_depth(interp(disp_lr, (H, W)))
            outputs[("depth", 0, scale)], outputs[("disp_scaled", 0, scale)] = depth, disp_scaled
            for i, f in enumerate(self.frame_ids):
                T = outputs[("cam_T_cam", 0, f)]
                cam_points = _backproject(depth, inv_K, pix)
                outputs[("cam_points", 0, scale)] = cam_points
                if self.bool_MotMask:
                    outputs[("motion_mask_r", f, scale)] = interp(outputs[("motion_mask", f, scale)], (H, W))
                else:
                    outputs[("motion_mask", f, scale)] = torch.ones(B, 1, h, w, device=disp0.device, dtype=disp0.dtype)
                    outputs[("motion_mask_r", f, scale)] = torch.ones(B, 1, H, W, device=disp0.device, dtype=disp0.dtype)
                if self.bool_CmpFlow:
                    sample_ego, ego_flow = _project(cam_points, K, T, H, W)
                    complete_flow = interp(outputs[("complete_flow", f, scale)], (H, W)).reshape(B, 3, -1)
                    residual_flow = complete_flow - ego_flow
                    independ_flow = residual_flow * outputs[("motion_mask_r", f, scale)].reshape(B, 1, -1)
                    outputs[("sample_ego", f, scale)] = sample_ego.detach()
                    tmp = torch.cat([cam_points.detach()[:, :3] + complete_flow, cam_points[:, 3:].detach()], 1)
                    outputs[("sample_complete", f, scale)] = _project(tmp, K, None, H, W)[0].detach()
                    if self.bool_MotMask:
                        moved = torch.cat([cam_points[:, :3] + independ_flow, cam_points[:, 3:]], 1)
                        sample, _ = _project(moved, K, T, H, W)
                    else:
                        moved = torch.cat([cam_points[:, :3] + complete_flow, cam_points[:, 3:]], 1)
                        sample, _ = _project(moved, K, None, H, W)
                else:
                    sample, ego_flow = _project(cam_points, K, T, H, W)
                    residual_flow = torch.zeros_like(ego_flow)
                    independ_flow = torch.zeros_like(ego_flow)
                outputs[("sample", f, scale)] = sample
                outputs[("color", f, scale)] = F.grid_sample(src[i], sample, padding_mode="border", align_corners=True)
                outputs[("ego_flow", f, scale)] = ego_flow
                outputs[("independ_flow", f, scale)] = independ_flow.reshape(B, 3, H, W)
                outputs[("residual_flow", f, scale)] = interp(residual_flow.reshape(B, 3, H, W), (h, w))
                if self.bool_automask:
                    outputs[("color_identity", f, scale)] = src[i]

    def _generate_kernels(self, outputs, K, inv_K, src, B, H, W):
        dev, NF = K.device, len(self.frame_ids)
        mode = (2 if self.bool_MotMask else 1) if self.bool_CmpFlow else 0
        f32 = lambda t: t if t.dtype == torch.float32 and t.is_contiguous() else t.float().contiguous()
        srcs = torch.stack(src)
        T = torch.stack([outputs[("cam_T_cam", 0, f)] for f in self.frame_ids])
        maps = [f32(outputs[("disp", 0, s)]) for s in range(NUM_SCALES)]
        if mode >= 1:
            maps += [f32(outputs[("complete_flow", f, s)]) for s in range(NUM_SCALES) for f in self.frame_ids]
        if mode >= 2:
            maps += [f32(outputs[("motion_mask", f, s)]) for s in range(NUM_SCALES) for f in self.frame_ids]
        out = _ViewSynth.apply(mode, f32(K), f32(inv_K), f32(srcs), f32(T), *maps)
        color = out[0]
        n_res = NUM_SCALES * NF if mode >= 1 else 0
        res = out[1:1 + n_res]
        sample, depth = out[1 + n_res], out[2 + n_res]
        self._fused = (color, srcs)
        for s in range(NUM_SCALES):
            h, w = H >> s, W >> s
            outputs[("depth", 0, s)] = depth[s]
            outputs[("disp_scaled", 0, s)] = 1 / depth[s]
            for i, f in enumerate(self.frame_ids):
                if self.bool_MotMask:
                    outputs[("motion_mask_r", f, s)] = interp(outputs[("motion_mask", f, s)], (H, W)).detach()
                else:
                    outputs[("motion_mask", f, s)] = torch.ones(B, 1, h, w, device=dev)
                    outputs[("motion_mask_r", f, s)] = torch.ones(B, 1, H, W, device=dev)
                outputs[("sample", f, s)] = sample[s, i]
                outputs[("color", f, s)] = color[s, i]
                if mode >= 1:
                    outputs[("sample_ego", f, s)] = out[3 + n_res][s, i]
                    outputs[("sample_complete", f, s)] = out[4 + n_res][s, i]
                    outputs[("residual_flow", f, s)] = interp(res[s * NF + i], (h, w))
                else:
                    outputs[("residual_flow", f, s)] = torch.zeros(B, 3, h, w, device=dev)
                if self.bool_automask:
                    outputs[("color_identity", f, s)] = src[i]

    # ---- losses -------------------------------------------------------------------------------------------------------------------------
    def compute_reprojection_loss(self, pred, target):
        l1 = torch.abs(target - pred).mean(1, True)
        return 0.85 * self.ssim(pred, target).mean(1, True) + 0.15 * l1

    def get_ground_depth(self, plane_param, inv_K, scale, outputs):
        B, _, h, w = outputs[("disp", 0, scale)].shape
        v = torch.matmul(inv_K[:, :3, :3], self.pix_coords(scale, inv_K)[None])
        w1, w2, w3 = plane_param[:, 0:1], plane_param[:, 1:2], plane_param[:, 2:3]
        ground_depth = (w3 / (v[:, 1:2] - v[:, 0:1] * w1 - v[:, 2:3] * w2)).reshape(B, 1, h, w)
        ground_depth = torch.where(torch.logical_or(ground_depth < 0, ground_depth > 100), torch.full_like(ground_depth, 100.0), ground_depth)
        return depth_to_disp(ground_depth), ground_depth

    def process_ground(self, inputs, outputs, scale=0, samples=None):
        """Plane distance, disparity minus the ground's disparity, and the ground mask at one scale (monodepth_loss.py:682-701)."""
        disp = outputs[("disp", 0, scale)]
        _, depth = disp_to_depth(disp)
        inv_K = torch.stack([i["inv_K"] for i in inputs]).to(disp.dtype)
        h, w = disp.shape[-2:]
        with torch.no_grad():
            cam_points = _backproject(depth, inv_K, self.pix_coords(scale, disp))
            if samples is None:
                samples = self.draw_ground_samples(disp.shape[0], h, w, disp.device)
            plane_dist, plane_param = self.gplane(cam_points[:, :3].reshape(-1, 3, h, w), samples)
            g_mask = (torch.abs(plane_dist) < self.gp_tol).to(disp.dtype)
            shifted = torch.cat([plane_param[:, :2], plane_param[:, 2:] + self.gp_tol], 1)
            ground_disp, ground_depth = self.get_ground_depth(shifted, inv_K, scale, outputs)
        disp_diff = torch.where(ground_depth == 100.0, torch.zeros_like(disp), disp - ground_disp)
        return plane_dist, disp_diff, g_mask

    def draw_ground_samples(self, B, h, w, device):
        n = self.gp_num_points_per_it * self.gp_max_it
        return torch.randint(0, self.gplane.num_ground_points(h, w), (B, n), generator=self.generator(device), device=device)

    def draw_tie_noise(self, B, H, W, device, dtype=torch.float32):
        return torch.randn((NUM_SCALES, B, len(self.frame_ids), H, W), generator=self.generator(device), device=device, dtype=dtype)

    def loss_coefs(self):
        out = {}
        for term in LOSS_TERMS:
            name = "g_" + term
            val = COEFS[name]
            if name in WEIGHT_RAMP:
                val *= np.clip(3 * self.step / 8_000, 0.0, 1.0) if self.phrage in ["mask init", "finetune"] else np.clip(3 * self.step / 35_000, 0.0, 1.0)
            out[term] = val
        return out

    def _photo_torch(self, inputs, outputs, scale, noise):
        target = torch.stack([i[("color", 0, 0)] for i in inputs])
        combined = torch.cat([self.compute_reprojection_loss(outputs[("color", f, scale)], target) for f in self.frame_ids], 1)
        if self.bool_automask:
            ident = torch.cat([self.compute_reprojection_loss(outputs[("color_identity", f, scale)], target) for f in self.frame_ids], 1)
            combined = torch.cat((ident + noise.to(ident.dtype) * TIE_NOISE_SCALE, combined), dim=1)
        to_optimise, idxs = torch.min(combined, dim=1)
        return to_optimise.mean(), idxs

    def compute_losses(self, inputs, outputs, tie_noise: Optional[Sequence[torch.Tensor]] = None,
                       ground_samples: Optional[Sequence[torch.Tensor]] = None):
        """The reference's loss dictionary (monodepth_loss.py:703-839): `loss_term/<name>`, `loss_term/<scale>`, `loss_coef/<name>`, `loss`."""
        losses = {"loss": 0}
        for term in LOSS_TERMS + list(range(NUM_SCALES)):
            losses[f"loss_term/{term}"] = 0
        for term, val in self.loss_coefs().items():
            losses[f"loss_coef/{term}"] = val
        color0 = torch.stack([i[("color", 0, 0)] for i in inputs])
        B, _, H, W = color0.shape
        NF = len(self.frame_ids)
        noise = None
        if self.bool_automask:
            noise = torch.stack(list(tie_noise)) if tie_noise is not None else self.draw_tie_noise(B, H, W, color0.device, color0.dtype)
            if tuple(noise.shape) != (NUM_SCALES, B, NF, H, W):
                raise ValueError(f"tie_noise: {NUM_SCALES} tensors of shape {(B, NF, H, W)} are needed")
        fused = self._fused
        self._fused = None
        if fused is not None:
            nz = None if noise is None else noise.to(device=color0.device, dtype=torch.float32).contiguous()
            p_photo, argmin = _PhotoLoss.apply(fused[0], color0.float().contiguous(), fused[1], nz)

        for scale in range(NUM_SCALES):
            ps = {k: 0 for k in LOSS_TERMS}
            h, w = outputs[("disp", 0, scale)].shape[-2:]
            color = F.interpolate(color0, [h, w], mode="bilinear", align_corners=False)
            if fused is not None:
                ps["p_photo"], idxs = p_photo[scale], argmin[scale]
            else:
                ps["p_photo"], idxs = self._photo_torch(inputs, outputs, scale, None if noise is None else noise[scale])
            if self.bool_automask:
                outputs["identity_selection/{}".format(scale)] = (idxs > NF - 1).float()

            if self.move_Depth:
                if losses["loss_coef/d_smooth"] > 0:
                    disp = outputs[("disp", 0, scale)]
                    norm_disp = disp / (disp.mean(2, True).mean(3, True) + 1e-7)
                    ps["d_smooth"] = compute_smooth_loss(norm_disp, color) / (2 ** scale)
                if losses["loss_coef/d_ground"] > 0 and self.bool_MotMask:
                    samples = None if ground_samples is None else ground_samples[scale]
                    _, disp_diff, _ = self.process_ground(inputs, outputs, scale=scale, samples=samples)
                    disp_diff = torch.where(disp_diff > 0, torch.zeros_like(disp_diff), disp_diff)
                    ps["d_ground"] = -1 * torch.mean(disp_diff) / (2 ** scale)

            for f in self.frame_ids:
                disp = outputs[("disp", 0, scale)]
                motion_mask = outputs[("motion_mask", f, scale)]
                h, w = motion_mask.shape[-2:]
                if self.move_CmpFlow and self.bool_CmpFlow:
                    complete_flow = outputs[("complete_flow", f, scale)]
                    residual_flow = outputs[("residual_flow", f, scale)]
                    if losses["loss_coef/c_smooth"] > 0:
                        ps["c_smooth"] = ps["c_smooth"] + compute_smooth_loss(complete_flow, color) / (2 ** scale) / NF
                    if self.bool_MotMask and losses["loss_coef/c_consistency"] > 0:
                        valid_disp = (disp > self.mask_disp_thrd).detach()
                        ps["c_consistency"] = ps["c_consistency"] + torch.mean(
                            valid_disp * (1 - motion_mask.detach()) * torch.abs(residual_flow)) / (2 ** scale) / NF
                if self.move_MotMask and self.bool_MotMask:
                    motion_prob = outputs[("motion_prob", f, scale)]
                    if losses["loss_coef/m_sparsity"] > 0:
                        sample_ego = interp(outputs[("sample_ego", f, scale)].permute(0, 3, 1, 2), (h, w))
                        sample_complete = interp(outputs[("sample_complete", f, scale)].permute(0, 3, 1, 2), (h, w))
                        disp_mag = torch.sum((sample_ego - sample_complete) ** 2, 1)
                        static = (disp_mag < disp_mag.mean()).unsqueeze(1)
                        count = static.sum((1, 2, 3))
                        every = (count > 0).all().to(motion_prob.dtype)                 # the reference's `if torch.all(...)` as a factor
                        soft = motion_prob.clamp(min=0) + torch.log1p(torch.exp(-motion_prob.abs()))    # BCE with logits against 0
                        bce = (soft * static).sum() / count.sum().clamp(min=1)
                        ps["m_sparsity"] = ps["m_sparsity"] + every * 3 * bce / (2 ** scale) / NF
                    if losses["loss_coef/m_smooth"] > 0:
                        ps["m_smooth"] = ps["m_smooth"] + compute_smooth_loss(motion_mask, color) / (2 ** scale) / NF

            for term in LOSS_TERMS:
                losses[f"loss_term/{scale}"] = losses[f"loss_term/{scale}"] + ps[term] * losses[f"loss_coef/{term}"]
                losses[f"loss_term/{term}"] = losses[f"loss_term/{term}"] + ps[term]
            losses["loss"] = losses["loss"] + losses[f"loss_term/{scale}"] / 4
        return losses

    def forward(self, outputs, targets, *args, tie_noise=None, ground_samples=None):
        self.generate_images_pred(outputs, targets)
        losses = self.compute_losses(targets, outputs, tie_noise=tie_noise, ground_samples=ground_samples)
        return {"loss_monodepth": losses["loss"]}
