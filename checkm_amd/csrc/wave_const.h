// wave_const.h -- the sizes that the byte-walking passes share, said once: host and device, no HIP.  The per-pass namespaces (ns, sw, rd,
// ub, aai, ol, mg, cv) refer to these; none repeats a literal.
#pragma once

namespace ckm {

constexpr int WAVE = 64;                         // lanes of a wavefront
constexpr int LANE_BYTES = 16;                   // one 128-bit load per lane
constexpr int WAVE_BYTES = LANE_BYTES * WAVE;    // one step of a wave over its text
constexpr int NKMER = 136;                       // canonical tetranucleotides: one row of counts, one signature

}  // namespace ckm
