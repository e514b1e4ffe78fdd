// The pair table of one strip, built by the workgroup's threads: one thread per (pair row, query row). Included, as
// text, by the four pair-table kernels where they build their table (as a function the loop comes out of the
// optimiser with its invariant sums associated differently, and the kernels' code objects change:
// profiles/pair_table_parts_device_code.txt). The including scope provides
//   gp                      the strip's profile rows: true scores as int16, row t at gp + t * a.qPad
//   kBuildThreads           threads of the workgroup
//   MIOPAL_PAIR_ENTRY(v)    the entry transform, true score -> what the kernel adds to a half
//                           (MIOPAL_SW_PAIR_ENTRY / MIOPAL_GLOBAL_PAIR_ENTRY, interseq_pair_parts.h)
// and pairs, nSym, a, R, SLOTS. Both targets' entries make ONE signed integer ("biased integer halves").
uint32_t* pw = reinterpret_cast<uint32_t*>(pairs);
const int total = nSym * nSym * R;
for (int idx = threadIdx.x; idx < total; idx += kBuildThreads) {
    const int row = idx / R, r = idx - row * R;
    const int tA = row / nSym, tB = row - tA * nSym;
    const int vA = gp[tA * a.qPad + r], vB = gp[tB * a.qPad + r];
    const int sA = MIOPAL_PAIR_ENTRY(vA);
    const int sB = MIOPAL_PAIR_ENTRY(vB);
    pw[row * (SLOTS * 4) + r] = (uint32_t)(sB * 65536 + sA);
}
