"""Four frames of a small scene with an environment bound and NO skybox (three serial, one split over two streams): the workload whose kernel names and counts
must be the same under this build of the library and under the parent commit's (BRMI_LIB_PATH), i.e. "off is off" at the level of launches.

    rocprofv3 --kernel-trace --output-format csv -d OUT_NEW -- python tools/envbuild_trace_frame.py
    BRMI_LIB_PATH=/path/to/parent/libbrmi.so rocprofv3 --kernel-trace --output-format csv -d OUT_PARENT -- python tools/envbuild_trace_frame.py
    python tools/kernel_trace_compare.py OUT_NEW OUT_PARENT
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    import torch
    from basicrenderer_amd import Scene
    from basicrenderer_amd.environment import Environment
    from basicrenderer_amd.renderer import VisibilityRenderer
    sc = Scene("tiny", 256, 144, point_lights=6, material_features=3)
    r = VisibilityRenderer(sc, occlusion=True)
    r.set_environment(Environment.procedural(16))
    for _ in range(3):
        r.execute()
    other = torch.cuda.Stream()
    r.execute(shading_stream=other)
    torch.cuda.synchronize()
    r.close()


if __name__ == "__main__":
    main()
