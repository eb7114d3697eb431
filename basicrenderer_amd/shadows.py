"""Light views for the spot / point shadow maps: the cameras the reference's light manager makes for a light, as the byte records
brmi_camera / brmi_culling_camera of include/brmi_types.h.  Host-side numpy only; the maps themselves are rendered and sampled by libbrmi.so.

Reference: LightManager::CreateSpotLightViewInfo / CreatePointLightViewInfo (view = XMMatrixLookToRH, up (0, 1, 0) for a spot light, GetCubemapViewMatrices for
the six faces) and GetProjectionMatrixForLight (XMMatrixPerspectiveFovRH(2 * acos(outerConeAngle) for a spot light, pi / 2 for a cube face, aspect 1,
nearPlane, farPlane): ordinary depth, not the main camera's reversed one)."""
import math

import numpy as np

LIGHT_POINT, LIGHT_SPOT, LIGHT_DIRECTIONAL = 0, 1, 2
CAMERA_BYTES, CULLING_CAMERA_BYTES = 736, 304
# brmi_light_info (include/brmi_types.h), 128 B
LIGHT_DTYPE = np.dtype([("type", "<u4"), ("innerConeAngle", "<f4"), ("outerConeAngle", "<f4"), ("shadowViewInfoIndex", "<i4"), ("posWorldSpace", "<f4", 4),
                        ("dirWorldSpace", "<f4", 4), ("attenuation", "<f4", 4), ("color", "<f4", 4), ("nearPlane", "<f4"), ("farPlane", "<f4"),
                        ("shadowMapIndex", "<i4"), ("shadowSamplerIndex", "<i4"), ("shadowCaster", "<u4"), ("boundingSphere", "<f4", 4), ("maxRange", "<f4"),
                        ("shadowSourceRadius", "<f4"), ("shadowSourceAngleDegrees", "<f4")])
assert LIGHT_DTYPE.itemsize == 128
# GetCubemapViewMatrices: look directions and up vectors of the faces +X -X +Y -Y +Z -Z (the Z pair looks down -z / +z as the reference has it)
CUBE_TARGETS = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, -1), (0, 0, 1)]
CUBE_UPS = [(0, 1, 0), (0, 1, 0), (0, 0, 1), (0, 0, -1), (0, 1, 0), (0, 1, 0)]


def look_to_rh(eye, direction, up):
    """XMMatrixLookToRH as a row-vector matrix (float64)."""
    eye, d, up = (np.asarray(v, dtype=np.float64) for v in (eye, direction, up))
    z = -d / np.linalg.norm(d)
    x = np.cross(up, z)
    if np.linalg.norm(x) < 1e-6:      # a light that looks along its up vector (the reference's matrix is not finite there): any other up will do
        x = np.cross((0.0, 0.0, 1.0), z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    m = np.eye(4)
    m[:3, 0], m[:3, 1], m[:3, 2] = x, y, z
    m[3, :3] = [-np.dot(x, eye), -np.dot(y, eye), -np.dot(z, eye)]
    return m


def perspective_fov_rh(fov, aspect, near, far):
    """XMMatrixPerspectiveFovRH(fov, aspect, NearZ = near, FarZ = far) as a row-vector matrix (float64)."""
    h = math.cos(0.5 * fov) / math.sin(0.5 * fov)
    m = np.zeros((4, 4))
    m[0, 0], m[1, 1] = h / aspect, h
    m[2, 2], m[2, 3], m[3, 2] = far / (near - far), -1.0, near * far / (near - far)
    return m


def light_camera(eye, direction, up, fov, near, far, resolution):
    """(brmi_camera bytes, brmi_culling_camera bytes) of a square light view: what CreateView leaves in the camera buffer for it."""
    view, proj = look_to_rh(eye, direction, up), perspective_fov_rh(fov, 1.0, near, far)
    world, vp = np.linalg.inv(view), view @ proj
    c = np.zeros(CAMERA_BYTES // 4, dtype=np.float32)
    c[0:3], c[3] = eye, 1.0
    for off, m in ((4, view), (20, world), (36, proj), (52, np.linalg.inv(proj)), (68, vp), (84, view), (100, proj), (116, proj), (132, proj)):
        c[off: off + 16] = m.reshape(-1)
    t = math.tan(0.5 * fov)
    planes = np.array([[0, 0, -1, -near], [0, 0, 1, far], [1, 0, -t, 0], [-1, 0, -t, 0], [0, 1, -t, 0], [0, -1, -t, 0]], dtype=np.float64)
    planes /= np.linalg.norm(planes[:, :3], axis=1, keepdims=True)
    c[148:172] = planes.reshape(-1)
    c[172:176] = [fov, 1.0, near, far]
    ci = c.view(np.uint32)
    c.view(np.int32)[176] = -1
    ci[177], ci[178], ci[179], ci[180] = resolution, resolution, int(resolution).bit_length(), 0
    p2 = 1 << (int(resolution) - 1).bit_length()
    c[181] = c[182] = resolution / p2
    cc = np.zeros(CULLING_CAMERA_BYTES // 4, dtype=np.float32)
    cc[0:4] = c[0:4]
    cc[4], cc[5], cc[6] = c[36], c[36 + 5], c[174]
    denom = np.float32(cc[5] * np.float32(0.5)) * np.float32(resolution)
    cc[7] = np.float32(1.0) / denom if denom > 0 else np.finfo(np.float32).max
    cc[12:15], cc[16:19], cc[20:23] = c[20:23], c[24:27], -c[28:31]      # the rows of viewInverse: right, up, -forward
    cc[24:40] = c[68:84]
    cc[40:44] = c[4:20].reshape(4, 4)[:, 2]
    cc[44:60], cc[60:76] = c[20:36], c[52:68]
    return c.view(np.uint8).copy(), cc.view(np.uint8).copy()


def light_views(light, resolution):
    """The light's views as [(camera bytes, culling-camera bytes)]: one for a spot light, six for a point light (+X -X +Y -Y +Z -Z).  `light`: a record of
    LIGHT_DTYPE."""
    pos = np.asarray(light["posWorldSpace"], dtype=np.float64)[:3]
    near, far = float(light["nearPlane"]), float(light["farPlane"])
    if int(light["type"]) == LIGHT_SPOT:
        fov = 2.0 * math.acos(min(1.0, max(-1.0, float(light["outerConeAngle"]))))
        return [light_camera(pos, np.asarray(light["dirWorldSpace"], dtype=np.float64)[:3], (0.0, 1.0, 0.0), fov, near, far, resolution)]
    if int(light["type"]) == LIGHT_POINT:
        return [light_camera(pos, t, u, 0.5 * math.pi, near, far, resolution) for t, u in zip(CUBE_TARGETS, CUBE_UPS)]
    raise ValueError("light_views: a spot or a point light")
