"""Temporal anti-aliasing, host side: the jitter sequence and the jittered camera record.

jitter_offset restates the reference's Halton and the DLSS branch of its UpscalingManager::GetJitter in fp32; jitter_camera applies an offset to a
brmi_camera / brmi_culling_camera pair the way the reference's renderer does before it uploads the primary camera: projection =
unjitteredProjection x Translation(jitterNDC), with viewProjection, projectionInverse and the culling camera derived from it as the scene library
derives them.  basicrenderer_amd/host/brmi_passes.hpp mirrors both for C++ hosts.
"""
import numpy as np

CAMERA_BYTES, CULLING_CAMERA_BYTES = 736, 304
# float offsets into brmi_camera (include/brmi_types.h)
_VIEW, _PROJECTION, _PROJECTION_INVERSE, _VIEW_PROJECTION = 4, 36, 52, 68
_PREV_JITTERED, _PREV_UNJITTERED, _UNJITTERED = 100, 116, 132
# ... and into brmi_culling_camera
_CULL_PROJ_X, _CULL_PROJ_Y, _CULL_VIEW_PROJECTION, _CULL_PROJECTION_INVERSE = 4, 5, 24, 60

_f32 = np.float32


def halton(i, b):
    """The reference's Halton(i, b): fp32 throughout."""
    f, r, i, bf = _f32(1.0), _f32(0.0), int(i), _f32(b)
    while i > 0:
        f = _f32(f / bf)
        r = _f32(r + _f32(f * _f32(i % b)))
        i = int(np.floor(_f32(_f32(i) / bf)))
    return r


def jitter_offset(frame_index, phases=16):
    """(jx, jy) in pixels, each in [-0.5, 0.5): (Halton(i + 1, 2) - 0.5, Halton(i + 1, 3) - 0.5) with i = frame_index % phases."""
    if phases <= 0:
        raise ValueError("jitter_offset: phases must be positive")
    i = int(frame_index) % int(phases)
    return float(_f32(halton(i + 1, 2) - _f32(0.5))), float(_f32(halton(i + 1, 3) - _f32(0.5)))


def jitter_ndc(jitter, width, height):
    """jitterNDC = (2 jx / W, -2 jy / H) in fp32."""
    jx, jy = _f32(jitter[0]), _f32(jitter[1])
    return float(_f32(_f32(_f32(2.0) * jx) / _f32(width))), float(_f32(_f32(_f32(-2.0) * jy) / _f32(height)))


def _m4(words, at):
    return words[at: at + 16].reshape(4, 4)


def jitter_camera(camera, culling_camera, width, height, jitter, previous=None, index=0):
    """Copies of the camera and culling-camera byte arrays with camera `index` jittered by `jitter` pixels.

    projection = unjitteredProjection x Translation(jitterNDC.x, jitterNDC.y, 0) (row vectors: the translation adds jitterNDC * w to clip x, y), rounded to
    fp32; viewProjection = view x projection and projectionInverse from the stored fp32 matrices in float64, rounded once, as the scene library does; the
    culling camera takes projX, projY, viewProjection and projectionInverse from there.  unjitteredProjection is untouched.  `previous` is the camera array
    this function returned for the frame before: prevJitteredProjection and prevUnjitteredProjection take its projection and unjitteredProjection; without
    it both keep what the record holds."""
    cam = np.array(camera, dtype=np.uint8, copy=True)
    cull = np.array(culling_camera, dtype=np.uint8, copy=True)
    c = cam[index * CAMERA_BYTES: (index + 1) * CAMERA_BYTES].view(np.float32)
    cc = cull[index * CULLING_CAMERA_BYTES: (index + 1) * CULLING_CAMERA_BYTES].view(np.float32)
    tx, ty = jitter_ndc(jitter, width, height)
    translate = np.eye(4, dtype=np.float64)
    translate[3, 0], translate[3, 1] = tx, ty
    projection = (_m4(c, _UNJITTERED).astype(np.float64) @ translate).astype(np.float32)
    _m4(c, _PROJECTION)[:] = projection
    _m4(c, _PROJECTION_INVERSE)[:] = np.linalg.inv(projection.astype(np.float64)).astype(np.float32)
    _m4(c, _VIEW_PROJECTION)[:] = (_m4(c, _VIEW).astype(np.float64) @ projection.astype(np.float64)).astype(np.float32)
    if previous is not None:
        p = np.asarray(previous, dtype=np.uint8)[index * CAMERA_BYTES: (index + 1) * CAMERA_BYTES].view(np.float32)
        _m4(c, _PREV_JITTERED)[:] = _m4(p, _PROJECTION)
        _m4(c, _PREV_UNJITTERED)[:] = _m4(p, _UNJITTERED)
    cc[_CULL_PROJ_X], cc[_CULL_PROJ_Y] = projection[0, 0], projection[1, 1]
    _m4(cc, _CULL_VIEW_PROJECTION)[:] = _m4(c, _VIEW_PROJECTION)
    _m4(cc, _CULL_PROJECTION_INVERSE)[:] = _m4(c, _PROJECTION_INVERSE)
    return cam, cull
