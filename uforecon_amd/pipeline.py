"""The reference's inference flow on this code base, under the reference's parameter names.

`UFOReconInference` = the per-ray mirror (`uforecon_amd.model.UFORecon`) + the per-frame producers
(`transmvsnet.feature` FeatureNet, `transmvsnet.FMT_with_pathway`, `transmvsnet.cost_regularization`,
`transmvsnet.DepthNet`, `feature_volume.cost_reg_2`) + the reference's dead `pre_conv` parameter: its state_dict has
exactly the reference model's 530 entries (tests/golden/reference_state_dict_shapes.json), so a reference checkpoint
loads with strict=True.  `extract_geometry` follows code1/model.py:760-842 end to end: images -> depth map files.
"""
from __future__ import annotations

import os

import numpy as np
import torch
import torch.nn as nn

from . import cascade, featurenet
from . import model as M


class UFOReconInference(M.UFORecon):
    def __init__(self, args, tune_convolutions: bool = True):
        super().__init__(args)
        if tune_convolutions:
            # the 3-D U-Nets are library convolutions: letting MIOpen search its algorithms once per shape halves them
            # (512x640: cascade 29 -> 19 ms, CostRegNetWeight 32 -> 17 ms); the first frame pays the search
            torch.backends.cudnn.benchmark = True
        self.transmvsnet = cascade.TransMVSNetCascade()
        self.transmvsnet.feature = featurenet.FeatureNet(base_channels=8)        # TransMVSNet.py:152
        self.feature_volume = cascade.MVSVolume(in_channels=1, base_channels=8)   # model.py:64
        self.pre_conv = nn.Conv2d(128, 32, 1, bias=False)                         # dead parameter of the reference
        self.eval()

    def train(self, mode: bool = True):
        """Inference only: the encoder's BatchNorms must run on their running statistics (in training mode they would
        normalise with batch statistics AND overwrite the loaded running_mean / running_var on every frame)."""
        if mode:
            raise M.UfrError("UFOReconInference is inference-only: it stays in eval mode (BatchNorm running statistics)")
        return super().train(False)

    # ---- model.py:139-160
    @staticmethod
    def build_pairs(imgs, proj_mats, depth_values):
        """imgs (B,N,3,H,W), proj_mats {stage: (B,N,2,4,4)}, depth_values (B,D) -> the N view rotations stacked on the batch
        axis: every source view is the reference view of one batch element."""
        N = imgs.shape[1]
        comb = np.array([list(range(i, N)) + list(range(0, i)) for i in range(N)])
        imgs = imgs[:, comb].reshape(-1, N, *imgs.shape[2:])                                   # (B*N, V, 3, H, W)
        pm = {st: proj_mats[st][:, comb].reshape(-1, N, 2, 4, 4) for st in ("stage1", "stage2", "stage3")}
        return imgs, pm, depth_values.expand(imgs.shape[0], -1)

    @torch.no_grad()
    def encode_frame(self, batch, cur_n_src_views=None):
        """model.py:775-806: everything `infer` needs besides the batch itself.  Returns (source_imgs_feat (B,V,32,h,w),
        feature_volume dict, match_feature list) and sets batch['depth_info'].  ``cur_n_src_views`` is what the caller hands
        `get_match_feat`: args.test_n_view by default (extract_geometry, model.py:785), args.train_n_view - 1 in validation
        (model.py:644).  = the frozen half, then the frustum build, both without gradients."""
        source_imgs_feat, cost_volumes, depth, match_feature = self.encode_frozen(batch, cur_n_src_views)
        frustums = self.build_frustums(batch, cost_volumes)
        self._set_depth_info(batch, depth)
        return source_imgs_feat, frustums, match_feature

    @torch.no_grad()
    def encode_frozen(self, batch, cur_n_src_views=None):
        """The half of `encode_frame` that `transmvsnet` computes (backbone, FMT, cascade) -- the half the reference freezes
        (model.py:72-87), always without gradients.  Returns (source_imgs_feat (B,V,32,h,w), {stage: cost volume}, the
        stage-3 depth, match_feature list)."""
        imgs, pm, dv = self.build_pairs(batch["source_imgs"], batch["proj_matrices"], batch["depth_values_org_scale"])
        H, W = imgs.shape[-2:]
        # TransMVSNet.py:175-178 runs the backbone on view v of every rotation, i.e. on each source image N times; one
        # pass over the N distinct images and a gather by the rotation table gives the same tensors
        B, N = batch["source_imgs"].shape[:2]
        comb = np.array([list(range(i, N)) + list(range(0, i)) for i in range(N)])
        base = self.transmvsnet.feature(batch["source_imgs"].reshape(B * N, *batch["source_imgs"].shape[2:]))
        feats = []
        for v in range(N):
            idx = torch.as_tensor([b * N + comb[r][v] for b in range(B) for r in range(N)], device=imgs.device)
            feats.append({st: base[st][idx] for st in ("stage1", "stage2", "stage3")})
        feats = self.transmvsnet.encode(feats, ref_idx=0)                                         # :181
        volume_info = self.transmvsnet(feats, pm, dv, (H, W))                                     # :183-236
        for f in feats:
            f["stage1"] = f["stage1"][0:1]                                                        # :782-783
        match_feature = self.transmvsnet.get_match_feat(feats, cur_n_src_views=self.args.test_n_view if cur_n_src_views is None else cur_n_src_views)   # :785
        source_imgs_feat = torch.stack([f["stage1"] for f in feats], dim=1)                       # :787-790
        cost_volumes = {st: volume_info[st]["cost_volume"] for st in ("stage1", "stage2", "stage3")}
        return source_imgs_feat, cost_volumes, volume_info["stage3"]["depth"], match_feature

    def build_frustums(self, batch, cost_volumes):
        """model.py:795-802 / 517-524: the three stages' feature and weight frustums from `feature_volume.cost_reg_2`, the one
        producer the reference trains.  Differentiable w.r.t. its parameters when gradients are on."""
        frustums = {}
        for st in ("stage1", "stage2", "stage3"):
            f, w = self.feature_volume(batch, cost_volumes[st])
            frustums[st] = {"feature_volume": f, "weight_volume": w}
        return frustums

    def _set_depth_info(self, batch, depth):
        if getattr(self.args, "mvs_depth_guide", 1) > 0:                                          # model.py:804-806 / 529-531
            batch["depth_info"] = (depth * batch["scale_factor"]).unsqueeze(0)

    @torch.no_grad()
    def extract_geometry(self, batch, batch_idx=0, out_dir=None, uniforms=None):
        """code1/model.py:760-842 (same name and role as the reference's hook; `out_dir` defaults to args.out_dir)."""
        source_imgs_feat, frustums, match_feature = self.encode_frame(batch)
        out_dir = out_dir if out_dir is not None else getattr(self.args, "out_dir", None)
        return M.UFORecon.extract_geometry(self, batch, source_imgs_feat, frustums, match_feature, out_dir=out_dir,
                                           uniforms=uniforms)

    @torch.no_grad()
    def extract_similarity(self, batch, batch_idx=0, bound_min=(-1., -1., -1.), bound_max=(1., 1., 1.), resolution=512, threshold=0.99,
                           min_views=0, out_dir=None):
        """code1/model.py:844-888: the mean grouped cosine similarity of the frame's matching features on a ``resolution``^3
        grid over [bound_min, bound_max] (`similarity_field.similarity_field`), `fraction occupied` printed, marching cubes at
        ``threshold``.  ``min_views > 0`` masks voxels that fewer views see (off = the reference).  Three stated differences
        from the reference:
          * with ``out_dir`` the mesh goes to ``<out_dir>/sim_<scan>_<resolution>.ply`` through `tsdf.meshwrite`, in scene
            coordinates; the reference writes ``sim_<scan>_512.dae`` through PyMCubes into the working directory, in voxel
            indices.  Without ``out_dir`` no mesh is extracted.
          * the return value ``u`` (X,Y,Z) is a device tensor; the reference returns a numpy array.
          * ``threshold`` is honoured; the reference overwrites its argument with 0.99, which is the default here."""
        from . import similarity_field as SF

        source_imgs_feat, frustums, match_feature = self.encode_frame(batch)
        fh = self.frame_handle(batch, source_imgs_feat, frustums, match_feature)
        u = SF.similarity_field(fh, bound_min, bound_max, resolution, min_views=min_views)
        print("fraction occupied", float((u > threshold).float().mean()))
        if out_dir is not None:
            verts, faces, normals = SF.field_mesh(u, bound_min, bound_max, level=threshold)
            print("done", tuple(verts.shape), tuple(faces.shape))
            os.makedirs(out_dir, exist_ok=True)
            SF.write_mesh(os.path.join(out_dir, "sim_%s_%s.ply" % (SF.scan_name(batch), SF.resolution_tag(resolution))), verts, faces, normals)
        return u

    @torch.no_grad()
    def validation_step(self, batch, batch_idx=0, logdir=None, uniforms=None):
        """code1/model.py:607-758 for a train-layout batch (dtu_train.py:442-495) of one frame: the reference view rendered
        in full through both passes and scored against the ground truth.  Returns the reference's dict -- val/loss_rgb_coarse,
        val/loss_rgb_fine, val/loss_depth_coarse, val/loss_depth_fine, psnr/coarse, psnr/fine (floats) and val/variance -- and
        writes its three files under ``logdir`` (default args.logdir; None: no files)."""
        if batch["source_imgs"].shape[0] != 1:
            raise M.UfrError(f"validation_step: one frame per call (B=1), got B={batch['source_imgs'].shape[0]}: the reference's own "
                             "file writing reads element 0 only")
        source_imgs_feat, frustums, match_feature = self.encode_frame(batch, cur_n_src_views=self.args.train_n_view - 1)
        logdir = logdir if logdir is not None else getattr(self.args, "logdir", None)
        return self.validation_frame(batch, source_imgs_feat, frustums, match_feature, logdir=logdir, uniforms=uniforms)

    @staticmethod
    def validation_epoch_end(batch_parts):
        """code1/model.py:578-604: the plain means of the frames' scores under the names the reference logs, and its return
        value ``loss`` = val/rgb_coarse + val/rgb_fine."""
        if not batch_parts:
            raise M.UfrError("validation_epoch_end: no frames")
        mean = lambda k: sum(p[k] for p in batch_parts) / len(batch_parts)  # noqa: E731
        out = {"psnr/coarse": mean("psnr/coarse"), "psnr/fine": mean("psnr/fine"), "val/rgb_coarse": mean("val/loss_rgb_coarse"),
               "val/rgb_fine": mean("val/loss_rgb_fine"), "val/loss_depth_coarse": mean("val/loss_depth_coarse"),
               "val/loss_depth_fine": mean("val/loss_depth_fine")}
        out["loss"] = out["val/rgb_coarse"] + out["val/rgb_fine"]
        return out


class UFOReconTraining(UFOReconInference):
    """The reference's training flow (code1/model.py:72-87, 492-575) on this code base: `configure_optimizers` and
    `training_step` for one frame per step.

    One stated difference from the reference: `train()` leaves `transmvsnet` in eval mode.  Under Lightning's `model.train()`
    the reference's FROZEN TransMVSNet runs its BatchNorms on batch statistics and overwrites the checkpoint's running
    statistics on every step, although none of its parameters train.  Here the frozen encoder stays on its running statistics
    (`FeatureNet` and `CostRegNet` are inference-only kernels with the BatchNorms folded in), and its parameters and buffers
    come out of training bit-identical."""

    def train(self, mode: bool = True):
        M.UFORecon.train(self, mode)          # the ray path and feature_volume
        self.transmvsnet.eval()               # ... and never the frozen encoder
        return self

    def configure_optimizers(self):
        """model.py:72-87: every `transmvsnet` parameter frozen, Adam over all others (the dead `pre_conv` among them: it never
        gets a gradient, so it never gets a state or an update) at args.uforecon_lr."""
        from . import optim

        rest = []
        for name, p in self.named_parameters():
            if "transmvsnet" in name:
                p.requires_grad = False
            else:
                rest.append(p)
        return optim.Adam(rest, lr=self.args.uforecon_lr)

    def training_step(self, batch, batch_idx=0, ray_idx=None, uniforms=None, generator=None):
        """model.py:492-575 for one frame (B = 1) -> ``(loss, log)``: the frozen half without gradients, the three frustums
        WITH, the ray draw, `infer`, `training_loss`.  ``ray_idx`` (1,RN) int64 and ``uniforms`` = (U1 (SN,RN), U2 (PN,RN)) pin
        the step's randomness; by default the rays are `ops.select_rays` of H W device uniforms (model.py:537: the first
        train_ray_num of their stable argsort) and the samplers' uniforms device draws, all from ``generator`` (a device
        generator; None: the device's default).  ``log``: what the reference logs -- train/depth_ray_coarse, train/depth_ray_fine,
        train/rgb_coarse, train/rgb_fine, train/loss_all, train/variance -- as detached device tensors: nothing in the step
        waits for the device."""
        B, _, _, H, W = batch["source_imgs"].shape
        if B != 1:
            raise M.UfrError(f"training_step: one frame per call (B=1), got B={B}: the frustum build and the ray draw are per frame")
        dev = batch["source_imgs"].device
        source_imgs_feat, cost_volumes, depth, match_feature = self.encode_frozen(batch, cur_n_src_views=self.args.train_n_view - 1)
        frustums = self.build_frustums(batch, cost_volumes)
        self._set_depth_info(batch, depth)
        if ray_idx is None:
            from . import ops

            ray_idx = ops.select_rays(torch.rand(H * W, device=dev, generator=generator), self.args.train_ray_num)[None]
        if uniforms is None:
            RN = ray_idx.shape[1]
            uniforms = (torch.rand(self.point_num, RN, device=dev, generator=generator),
                        torch.rand(self.point_num_2, RN, device=dev, generator=generator))
        r = self.infer(batch, ray_idx, source_imgs_feat, frustums, match_feature=match_feature, uniforms=uniforms)
        loss, parts = self.training_loss(r, batch)
        log = {"train/" + k: v for k, v in parts.items()}
        log["train/loss_all"] = loss.detach()
        log["train/variance"] = r[16].detach()
        return loss, log
