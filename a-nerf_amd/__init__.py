"""MI355X-native A-NeRF render path: drop-in RayCaster / render / render_path over HIP kernels.

Import as ``importlib.import_module("a-nerf_amd")`` (the directory name is not a Python
identifier).  The compute lives in libanerf_hip.so (C ABI: include/anerf.h); this package is
the host-side mirror of the reference interface (core/raycasters.py, core/trainer.py,
run_nerf.py).
"""
from .config import RenderConfig, flops_per_sample, samples_per_ray
from .raycaster import RayCaster, create_raycaster, load_checkpoint
from .render import batchify_rays, render, render_path, render_frames
from .isosurface import isosurface, isosurface_reference, mesh_from_grid, read_ply, render_mesh, write_ply
from .meshops import (filter_mesh, mesh_components, mesh_components_reference, mesh_turntable, rasterize_mesh,
                      rasterize_mesh_reference, simplify_mesh, simplify_mesh_reference, smooth_mesh,
                      smooth_mesh_reference, turntable_transforms, vertex_adjacency, vertex_adjacency_reference,
                      vertex_normals, vertex_normals_reference, SimplifiedMesh, SIMPLIFY_MAX_CELLS, camera_view,
                      rasterize_mesh_camera, rasterize_mesh_camera_reference, render_mesh_views,
                      render_mesh_views_reference, MeshRaster, MeshViews)
from . import dataset, rays, synthetic, train, trainer
from .trainer import Adam, Trainer, create_popt, nerf_loss_reference, pose_loss_reference, adam_reference
from .dataset import RayImageDataset, RayImageSampler
from . import evaluation
from .evaluation import (EvalScores, evaluate_box_metric, evaluate_frames, evaluate_frames_reference, evaluate_metric,
                         render_testset)
from . import sequences
from .sequences import (RenderSequence, load_animate, load_bubble, load_bullettime, load_correction,
                        load_interpolate, load_pose_rotate, load_retarget, load_selected, matrix_to_axis_angle,
                        matrix_to_axis_angle_reference, pose_ckpt_to_pose_data, pose_sequence,
                        pose_sequence_reference, render_sequence, write_png)
from . import posescore
from .posescore import (PoseScores, Criterion_MPJPE, Criterion3DPose_ProcrustesCorrected,
                        Criterion3DPose_leastQuaresScaled, evaluate_pampjpe, evaluate_pampjpe_from_smpl_params,
                        evaluate_pose_ckpt, evaluate_pose_layer, evaluate_poses, evaluate_poses_reference, procrustes,
                        procrustes_align)
from . import preprocess
from .preprocess import (create_kp_mask, create_kp_masks, create_kp_masks_reference, dilate_masks,
                         dilate_masks_reference, draw_segments, draw_segments_reference, draw_skeleton2d,
                         draw_skeletons, draw_skeletons_3d, draw_skeletons_3d_reference, draw_skeletons_reference,
                         erode_masks, erode_masks_reference, mask_morph, mask_morph_reference, median_backgrounds,
                         median_backgrounds_reference, prepare_dataset, sampling_masks, sampling_masks_reference,
                         skeleton3d_to_2d, skeleton3d_to_2d_reference)

__all__ = ["RenderConfig", "RayCaster", "create_raycaster", "load_checkpoint", "render", "render_path",
           "render_frames", "batchify_rays", "rays", "synthetic", "dataset", "RayImageDataset", "RayImageSampler", "flops_per_sample", "samples_per_ray",
           "isosurface", "isosurface_reference", "mesh_from_grid", "read_ply", "render_mesh", "write_ply",
           "mesh_components", "mesh_components_reference", "filter_mesh", "vertex_adjacency",
           "vertex_adjacency_reference", "smooth_mesh", "smooth_mesh_reference", "vertex_normals",
           "vertex_normals_reference", "rasterize_mesh", "rasterize_mesh_reference", "mesh_turntable",
           "turntable_transforms", "simplify_mesh", "simplify_mesh_reference", "SimplifiedMesh",
           "SIMPLIFY_MAX_CELLS", "camera_view", "rasterize_mesh_camera", "rasterize_mesh_camera_reference",
           "render_mesh_views", "render_mesh_views_reference", "MeshRaster", "MeshViews", "trainer", "Adam", "Trainer",
           "create_popt", "nerf_loss_reference", "pose_loss_reference", "adam_reference", "evaluation", "EvalScores",
           "evaluate_frames", "evaluate_frames_reference", "evaluate_metric", "evaluate_box_metric", "render_testset",
           "sequences", "RenderSequence", "pose_sequence", "pose_sequence_reference", "render_sequence", "write_png",
           "matrix_to_axis_angle", "matrix_to_axis_angle_reference", "pose_ckpt_to_pose_data", "load_retarget",
           "load_bullettime", "load_pose_rotate", "load_interpolate", "load_animate", "load_bubble", "load_selected",
           "load_correction", "posescore", "PoseScores", "evaluate_poses", "evaluate_poses_reference",
           "procrustes_align", "procrustes", "Criterion_MPJPE", "Criterion3DPose_ProcrustesCorrected",
           "Criterion3DPose_leastQuaresScaled", "evaluate_pampjpe", "evaluate_pampjpe_from_smpl_params",
           "evaluate_pose_layer", "evaluate_pose_ckpt", "preprocess", "dilate_masks", "erode_masks", "sampling_masks",
           "mask_morph", "draw_segments", "skeleton3d_to_2d", "draw_skeleton2d", "draw_skeletons", "draw_skeletons_3d",
           "create_kp_masks", "create_kp_mask", "median_backgrounds", "prepare_dataset", "mask_morph_reference",
           "dilate_masks_reference", "erode_masks_reference", "sampling_masks_reference", "draw_segments_reference",
           "draw_skeletons_reference", "draw_skeletons_3d_reference", "skeleton3d_to_2d_reference",
           "create_kp_masks_reference", "median_backgrounds_reference"]
