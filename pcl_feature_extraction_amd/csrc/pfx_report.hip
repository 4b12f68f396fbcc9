// pfx_report.hip -- the deferred reports of the stream-ordered calls (pfx_internal.h, DESIGN.md "The
// descriptors' common frame"): the slots' device words, their copy to one pinned block in stream
// order, and their resolution after a synchronisation.
#include "pfx_internal.h"

namespace pfx {
namespace {

struct SlotInfo {
  const char* words;  // the name of the device words' buffer
  int sticky;         // the leading words that stand until they are reported
  void (*finish)(pfx_ctx*, const int*);
};
const SlotInfo kSlots[kReportSlots] = {
    {"fpfh_err", 1, fpfh_report},       {"pfh_err", 1, pfh_report},     {"spin_err", 4, spin_report},
    {"igrad_err", 4, igrad_report},     {"rift_err", 4, rift_report},   {"ispin_err", 4, ispin_report},
    {"sc_err", 4, sc_report},           {"sc_lrf_err", 4, lrf_report},  {"moments_err", 4, moments_report},
    {"pcurv_err", 4, pcurv_report},     {"board_err", 4, board_report}, {"boundary_err", 0, boundary_report},
    {"narf_desc_err", 0, narf_desc_report},
};

}  // namespace

int* report_words(pfx_ctx* ctx, ReportSlot slot, bool clear_per_call) {
  DevBuf& eb = ctx->buf(kSlots[slot].words);
  const bool fresh = !eb.ptr;
  int* w = eb.as<int>(kReportWords);
  const int keep = fresh ? 0 : kSlots[slot].sticky;
  if (fresh || clear_per_call)
    PFX_HIP(hipMemsetAsync(w + keep, 0, (kReportWords - keep) * sizeof(int), ctx->stream));
  return w;
}

int* report_host(pfx_ctx* ctx, ReportSlot slot) {
  Reports& R = ctx->reports;
  if (!R.host)
    PFX_HIP(hipHostMalloc((void**)&R.host, sizeof(int) * kReportSlots * kReportWords, hipHostMallocDefault));
  return R.host + slot * kReportWords;
}

void report_post(pfx_ctx* ctx, ReportSlot slot, const int* words, int n) {
  PFX_HIP(hipMemcpyAsync(report_host(ctx, slot), words, sizeof(int) * n, hipMemcpyDeviceToHost, ctx->stream));
  ctx->reports.pending[slot] = true;
}

void reports_resolve(pfx_ctx* ctx, ReportSlot first, ReportSlot last) {
  for (int s = first; s <= last; ++s) {
    if (!ctx->reports.pending[s]) continue;
    ctx->reports.pending[s] = false;
    try {
      kSlots[s].finish(ctx, report_host(ctx, (ReportSlot)s));
    } catch (const Error&) {
      int* w = ctx->buf(kSlots[s].words).as<int>(kReportWords);
      PFX_HIP(hipMemsetAsync(w, 0, kSlots[s].sticky * sizeof(int), ctx->stream));  // reported once
      throw;
    }
  }
}

}  // namespace pfx
