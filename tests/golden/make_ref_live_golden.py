#!/usr/bin/env python
"""Digests of what the reference's OWN CPU code (oracle/_ref, rendered from the reference's source where it lies; needs
the reference checkout) makes of the seeded inputs of the three tests of tests/test_oracle.py that also run against the
live library:

    python tests/golden/make_ref_live_golden.py     ->  tests/golden/ref_live_digests.json

  rulebook_sweep      out_inds / pair / num of the 40 random rulebook problems (null: the reference refuses the case)
  native_loop         forward, input and weight gradient of the per-offset conv loop with the reference's GatherCPU
                      switched in, on dyadic values (every sum exact in fp32: independent of the GEMM's order)
  point2voxel         voxels / coordinates / point counts of Point2VoxelCPU, plain and mean, three point clouds
  maxpool             IndiceMaxPoolCPU forward and backward

The tests compare oracle.cpp's restatement with these digests on any box, and with the library itself where it exists."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
from oracle import ref  # noqa: E402
import oracle  # noqa: E402
from golden import digest, native_loop_cases, rulebook_sweep_cases, section_8f_inputs  # noqa: E402


def main():
    assert ref.build() is not None, "oracle/_ref needs the reference checkout"
    out = {"rulebook_sweep": []}
    for idx, bs, shape, ksize, stride, pad, dil, subm, transposed in rulebook_sweep_cases():
        try:
            want = ref.get_indice_pairs(idx, bs, shape, ksize, stride, pad, dil, None, subm, transposed)
        except (ValueError, RuntimeError):
            out["rulebook_sweep"].append(None)
            continue
        out["rulebook_sweep"].append([digest(a) for a in want[:3]])
    out["native_loop"] = {}
    for key, out_inds, pair, num, subm, f, w, g in native_loop_cases(dyadic=True):
        oracle.use_reference_gather(True)
        try:
            y = oracle.indice_conv(f, w, pair, num, out_inds.shape[0], subm=subm)
            din, dw = oracle.indice_conv_backward(f, w, g, pair, num, subm=subm)
        finally:
            oracle.use_reference_gather(False)
        out["native_loop"][key] = [digest(t.numpy()) for t in (y, din, dw)]
    p2v, (pair, num, n_out, f, dout) = section_8f_inputs()
    out["point2voxel"] = [[digest(*ref.point2voxel(pts, vs, cr, grid, cap, 4, mean)) for mean in (False, True)]
                          for pts, vs, cr, grid, cap in p2v]
    pooled = ref.indice_maxpool(f, pair, num, n_out)
    out["maxpool"] = [digest(pooled), digest(ref.indice_maxpool_backward(f, pooled, dout, pair, num))]
    with open(os.path.join(HERE, "ref_live_digests.json"), "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("wrote", os.path.join(HERE, "ref_live_digests.json"))


if __name__ == "__main__":
    main()
