// acq_knobs.hip - the acquisition planners' switches: the ONE definition of the state acq_host.h declares, and the test build's
// setters that write it.  Kept out of acq.hip (a new knob leaves the scorer file, and with it the traffic record's hash, alone) and out
// of every header (a copy per source would let a setter in one source miss the reader in another).
#include "acq_host.h"

namespace pp {

AcqKnobs g_knobs;
thread_local int t_exact_call = 0;

#ifdef PP_DEBUG_KNOBS
extern bool g_diverse_stream;     // acq_select.hip (pp_debug_set_acq_tuning value 11 of `occ`)
#endif

}  // namespace pp

using namespace pp;

extern "C" {

#ifdef PP_DEBUG_KNOBS
void pp_debug_set_reduce_mode(int mode)
{
    g_knobs.large_multiblock = (mode & 256) ? 0 : 1;      // bit 8: large-k selection through the one-block-per-image radix select (A/B)
    g_knobs.large_q = (mode & 512) ? 0 : 1;               // bit 9: no quantised-histogram select where the score range is known (A/B)
    g_knobs.hist_fuse = (mode & 1024) ? 0 : 1;            // bit 10: the score histogram in its own pass over the map (select_qhist_kernel), not in the scorer launch
    g_knobs.generic_q = (mode & (1 << 22)) ? 0 : 1;       // bit 22: maps without a known range (pp_topk_select) through the four-pass radix select
    g_knobs.emit = (mode & 2048) ? 0 : 1;                 // bit 11: no sampled-threshold candidate emission (the map-writing scorer + topk_qsel_kernel)
    g_knobs.emit_mult16 = ((mode >> 12) & 63) ? ((mode >> 12) & 63) : 40;    // bits 12-17: the sample aims at this / 16 x k passing pixels
    { static const int locs[4] = {128, 64, 256, 512}, gpl[4] = {4, 2, 1, 8};
      g_knobs.sample_locs = locs[(mode >> 18) & 3]; g_knobs.sample_gpl = gpl[(mode >> 20) & 3]; }      // bits 18-21: the sample's shape
    mode &= 255;
    g_knobs.reduce_mode = (mode >= 0 && mode <= 2) ? mode : 0;
}

void pp_debug_set_exact_formula(int on) { g_knobs.exact_formula = on ? 1 : 0; }

void pp_debug_set_lsel_probe(void* device_buffer) { g_knobs.lsel_probe = reinterpret_cast<uint32_t*>(device_buffer); }

void pp_debug_set_acq_tuning(int occ, int ppt)
{
    g_knobs.tune_xcd = (occ >> 8) & 3;
    g_knobs.acq_strat_spec = (occ >> 10) & 1 ? 0 : 1;
    g_knobs.nt_off = (occ >> 11) & 1;
    occ &= 0xFF;
    g_knobs.tune_occ = (occ == 2 || occ == 3 || occ == 4 || occ == 8 || occ == 9 || occ == 10) ? occ : 0;   // 10: streamed class vector at any C (A/B, tests)
    g_diverse_stream = occ == 11;                   // 11: pp_diverse_select's streaming form at any M (acq_select.hip owns the flag)
    g_knobs.tune_ppt = (ppt == 4 || ppt == 8) ? ppt : 0;
}
#endif

}  // extern "C"
