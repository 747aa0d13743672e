// shared_plan_check.cpp -- prints shared_plan (facedeform_amd/csrc/fd_shared_plan.h, included alone) for every shape of the
// table tests/golden/shared_plan_table.txt was recorded for, one line per (Mpad, nF, kind) with every field of the plan:
//     g++ -std=c++17 -I facedeform_amd/csrc tests/tools/shared_plan_check.cpp -o shared_plan_check && ./shared_plan_check
// tests/test_shared_plan.py builds it and compares the lines with the table.
#include <cstdio>

#include "fd_shared_plan.h"

int main()
{
    const int kinds[2] = {2, 1};        // FD_KERNEL_THIN_PLATE, FD_KERNEL_GAUSSIAN_QNN (include/facedeform_hip.h)
    int mpads[43], n = 0;
    for (int m = 16; m <= 640; m += 16) mpads[n++] = m;
    mpads[n++] = 1024; mpads[n++] = 2048; mpads[n++] = 4096;
    for (int k = 0; k < 2; ++k)
        for (int i = 0; i < n; ++i)
            for (int nF = 1; nF <= 32; ++nF) {
                const fd::SharedPlan q = fd::shared_plan(mpads[i], nF, kinds[k]);
                // columns: Mpad nF kind variant ntiles nslot nkb kchunk poly_at copy_at norm_at wtile_bytes frame_bytes lds_fixed lds_per_kb
                //          threads group_vertices kernel
                printf("%d %d %d %d %d %d %d %d %zu %zu %zu %zu %zu %zu %zu %d %d %s\n",
                       mpads[i], nF, kinds[k], q.variant, q.ntiles, q.nslot, q.nkb, q.kchunk, q.poly_at, q.copy_at, q.norm_at, q.wtile_bytes,
                       q.frame_bytes, q.lds_fixed, q.lds_per_kb, q.threads, q.group_vertices, q.kernel);
            }
    return 0;
}
