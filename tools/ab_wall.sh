#!/bin/bash
# A/B of library builds by wall time per frame (tools/frame_wall.py: the bench's shape, 64 frames
# per launch, one launch in flight), alternating builds, two passes per config.  Usage (GPU box):
#   bash tools/ab_wall.sh "C2 C3 C4" lib/ab/libraytracer_hip_X.so lib/libraytracer_hip.so ...
# EXTRA="--strip spheres" etc. is passed to frame_wall.py.  A library given as VAR=VALUE,path runs with that
# variable set (a switch of the same build as a leg of its own: RT_PRIM_FOOT=0,lib/libraytracer_hip.so).
set -u -o pipefail  # (a leg that fails ends the run: nothing more starts on the GPU)
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
cfgs=$1; shift
for c in $cfgs; do
    for rep in 1 2; do
        for leg in "$@"; do
            lib=${leg##*,}
            setenv=
            if [ "$lib" != "$leg" ]; then setenv=${leg%,*}; echo -n "[$setenv] "; fi
            timeout -k 10 180 env $setenv python tools/frame_wall.py --config "$c" --inflight ${INFLIGHT:-1} --batch ${BATCH:-64} --frames 1024 \
                --lib "uu-infogr-raytracer_amd/$lib" ${EXTRA:-} 2>&1 | grep -v amdgpu.ids || exit $?
        done
    done
done
