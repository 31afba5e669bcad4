"""What the trainer's fused sum phase costs: the workload for one `rocprofv3 --kernel-trace --stats` pass.

    rocprofv3 --kernel-trace --stats -f csv -d OUT -o pq_train -- python tools_dev/profile_pq_train.py [rows] [dim] [M] [iters] [calls]
                                                                          (defaults: 262144 768 48 4 3)

`calls` times: pq_train over every row of a synthetic fp16 corpus (iters dispatches of pq_train_step_kernel each), then pq_build
under the trained codebooks (one grid of pq_encode_kernel over the SAME rows: the cost of the assignment alone).  In the kernel
statistics, the average duration of pq_train_step_kernel over that of pq_encode_kernel is what assignment + sums cost relative to
the assignment.  Prints the shapes and the bytes / fmas of one iteration, computed from them."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nano-vectordb_amd"))
import nvdb_amd  # noqa: E402


def main():
    a = [int(x) for x in sys.argv[1:]]
    rows, dim, M, iters, calls = (a + [262144, 768, 48, 4, 3][len(a):])[:5]
    ctx = nvdb_amd.HipContext(0)
    ctx.generate_corpus(20240613, rows, dim, nvdb_amd.DT_F16)
    for _ in range(calls):
        cb, err = ctx.pq_train(M, iters, 7, want_err=True)
        ctx.pq_build(cb)
    chunks = -(-rows // 4096)
    print(json.dumps(dict(rows=rows, dim=dim, M=M, iters=iters, calls=calls, out_err=err.tolist(),
                          per_iteration=dict(fmas=rows * dim * 256, f32_row_bytes_read=rows * dim * 4,
                                             partial_bytes_written=chunks * 256 * dim * 8 + chunks * M * 256 * 4))))
    ctx.close()


if __name__ == "__main__":
    main()
