"""Rendering of SDFNet shapes (the reference's rendering/ package without its OpenGL viewer): raymarching.render_image and the
camera helpers of rendering/math.py.  The sphere tracer runs on the device (csrc/raymarch.hip)."""
