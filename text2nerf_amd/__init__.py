"""MI355X-native TensoRF VM-split ray-marching renderer (the Text2NeRF hot path).

Host-side mirror of the reference interface for this path; the arithmetic runs in libt2n_hip.so (include/t2n.h).
"""
from .renderer import (OctreeRender_trilinear_fast, SimpleSampler, BatchPrefetcher, render_views, postprocess_frame,  # noqa: F401
                       evaluation_frames, evaluation, evaluation_path, render_geometry_views)
from .tensorf import Geometry  # noqa: F401
from .tensorf import (AlphaGridMask, MLPRender, MLPRender_Fea, MLPRender_Fea_noview, MLPRender_PE, RGBRender, SHRender, TensorBase,  # noqa: F401
                      TensorCP, TensorVM, TensorVMSplit, positional_encoding, raw2alpha, release_workspaces, to_device_async,
                      workspace_reserved)
from .ray_utils import (get_ray_directions, get_ray_directions_blender, get_rays, generate_rays, dda, ray_marcher,  # noqa: F401
                        ndc_rays_blender, ndc_rays, sample_pdf, depth2dist, ndc2dist)
from .sh import eval_sh_bases  # noqa: F401
from .dataset import DeviceTrainSet  # noqa: F401
from .mesh import Mesh, marching_cubes, convert_sdf_samples_to_ply, write_ply  # noqa: F401
from .mesh import Components, mesh_components, filter_components  # noqa: F401
from .mesh import Adjacency, mesh_adjacency, smooth_mesh, vertex_normals  # noqa: F401
from .mesh import Clusters, mesh_clusters, simplify_mesh  # noqa: F401
from .mesh import select_faces  # noqa: F401
from .tsdf import TSDFVolume, tsdf_integrate, tsdf_mesh  # noqa: F401
from .volume import VolumeComponents, volume_components, filter_volume  # noqa: F401
from .tensorf import PruneReport  # noqa: F401
