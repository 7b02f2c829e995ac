"""Drop-in import surface: `from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer`
(render/render_3dgs.py:3-4 of the reference) resolves to the MI355X-native 3D-Gaussian ablation rasterizer."""
from gaus_slam_amd.rasterizer3d import GaussianRasterizationSettings, GaussianRasterizer  # noqa: F401
