// nvdb_insert.h -- what nvdb_insert.cpp shares with the index (nvdb_ivf.cpp): an insertion in its two halves.  The first checks the
// call and stages the new rows on the device, where nvdb_hip_ivf_add_rows assigns them to their lists; the second places them.
// Internal.
#pragma once
#include "nvdb_ctx.h"
#include "insert_plan.h"

namespace nvdbhip {

// the new rows (and the scales of an int8 corpus) on the device, for the length of one call
struct InsertStage {
  void* rows = nullptr;
  float* scales = nullptr;
  InsertStage() = default;
  InsertStage(const InsertStage&) = delete;
  InsertStage& operator=(const InsertStage&) = delete;
  ~InsertStage() { if (rows) (void)hipFree(rows); if (scales) (void)hipFree(scales); }
};

// Every check of nvdb_hip_insert_rows (context, corpus, ownership, pointers, the row limits, needs_table: a partition table is
// resident, part_of != nullptr: its entries name partitions) and then, for m > 0, the staging: a call that is refused has copied
// nothing.  *done: the call is answered (an error, or m == 0).  Nothing of the context changes.
nvdb_status insert_stage(nvdb_hip_ctx* c, const char* who, const void* rows, const float* scales, uint64_t m, bool needs_table, const uint32_t* part_of,
                         InsertStage& stage, bool* done);

// Places the staged rows: part_of as nvdb_hip_insert_rows takes it (its entries checked once more by the plan: the index's assignment comes this way only).  NVDB_ERR_HIP after the first row has moved: the
// context has dropped its corpus (c->rows == nullptr).
// out_plan (optional): the plan the move ran by, on success -- what an index spreads its permutation with.
nvdb_status insert_staged(nvdb_hip_ctx* c, const char* who, const InsertStage& stage, uint64_t m, const uint32_t* part_of, uint64_t* out_new_rows, uint64_t* out_n,
                          InsPlan* out_plan = nullptr);

}  // namespace nvdbhip
