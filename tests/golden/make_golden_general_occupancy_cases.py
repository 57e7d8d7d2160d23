"""Shared settings of tests/golden/make_golden_general_occupancy.py and the tests that read general_occupancy.npz: a wide VM-split field
(more components per plane than the tuned kernels hold, a 144-unit head) with an AlphaGridMask, regular and NDC rays. Importable
without the reference."""
GRID = [10, 9, 8]
AABB = [[-3.0, -2.5, -2.0], [3.0, 2.5, 4.0]]
NEAR_FAR = [0.3, 7.0]
MASK_GRID = (16, 14, 12)       # updateAlphaMask's gridSize
DENSE_GRID = (7, 6, 5)         # getDenseAlpha's gridSize
N_TRAIN = 40                   # N_samples of the train-mode renders
ALPHA_THRES = 0.05             # alphaMask_thres: a mask that keeps part of the box
SEEDS = {"mlp": 21, "fea": 22}
COMMON = dict(density_n_comp=[24, 20, 32], appearance_n_comp=[64, 72, 56], app_dim=27, featureC=144, pos_pe=0)
CASES = {
    "mlp": dict(COMMON, shadingMode="MLP_Fea_noview", fea_pe=2, view_pe=0),
    "fea": dict(COMMON, shadingMode="MLP_Fea", fea_pe=2, view_pe=2),      # view-dependent: the NDC direction normalisation
}
FIELD = dict(near_far=NEAR_FAR, alphaMask_thres=ALPHA_THRES, density_shift=-10, distance_scale=25, step_ratio=1.0,
             fea2denseAct="softplus")
DENSITY_SCALE = 0.8
CAMERA = dict(H=12, W=16, yaw=0.2, pitch=-0.1, center=(0.1, 0.2, -2.5))
NDC = dict(H=12, W=16, focal=14.0, near=1.0)   # ndc_rays_blender's arguments
