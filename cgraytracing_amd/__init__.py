"""cgraytracing_amd -- MI355X-native eye-ray pass of haoyuzhao123/CGRayTracing."""
from .scene import Bezier, Camera, Object, Plane, Sphere, Texture, TriangleMesh, Vec3  # noqa: F401

__all__ = ["Bezier", "Camera", "Object", "Plane", "Sphere", "Texture", "TriangleMesh", "Vec3", "Scene", "render", "tonemap_rgb8", "write_png", "camera_rays_host", "emit_photons_host", "math_probe"]


def __getattr__(name):
    # Scene / render need libcgrt.so; importing them lazily keeps `import cgraytracing_amd.scene` usable for
    # tools that only describe scenes.
    if name == "Scene":  # engine.Scene with the refit calls (refit.py) and the grid AOVs (aov.py)
        import importlib
        return importlib.import_module(__name__ + ".aov").Scene
    if name in ("render", "tonemap_rgb8", "write_png", "camera_rays_host", "emit_photons_host", "math_probe"):
        import importlib
        _r = importlib.import_module(__name__ + ".engine")
        return getattr(_r, name)
    raise AttributeError(name)
