// mh_select.hpp -- which codec kernel instance a plan launches, and with how much dynamic LDS.  Pure C++ (no HIP, no
// device code): muahuff.hip turns a pick into its template instance at plan creation; the kernels size their LDS areas with
// the helpers below, as their launches do; tests/planner_check.cpp --cells prints the picks under the sanitizers.
#pragma once
#include <stdint.h>

#include <string>

namespace mh {
constexpr int kDtab = 512;  // decode table bytes per channel (2^maxlen <= 512)
constexpr size_t kLds3PerCu = 41 * 1024;  // LDS request that leaves 3 workgroups per CU (dec_lds_bytes, enc_lds_bytes)

// LDS areas in dwords (the kernels index by the same functions).  Encoder, per wave: carried tail (64) + header room (32) + staging / image area
constexpr uint32_t enc2_wave_dwords(uint32_t stage_dw) { return 96 + stage_dw * 64; }
// A wave's tables in k_encode2w: the pair table has 4^PB entries -- 64 for S <= 8 -- plus the 16 single-symbol entries;
// the four-symbol table of 2-bit input has 256.  Sized exactly: with 3-bit pairs four workgroups fit a CU at the
// largest staging as well.
constexpr uint32_t enc2w_table_dwords(int PB, int PK) { return (PK == 2 ? 512u : 2u << (2 * PB)) + 32u; }
template <int PB, int PK> constexpr uint32_t enc2w_table_dwords() { return enc2w_table_dwords(PB, PK); }
template <int PB, int PK> constexpr uint32_t enc2w_wave_dwords(uint32_t dw) { return enc2w_table_dwords(PB, PK) + enc2_wave_dwords(dw); }
// decoder, workgroup-shared (per wave in k_decode2w) tables: multi-symbol table (2 dwords per entry for K = 4, 1 for
// the pair table) + the 512-byte per-symbol table used by partial / oversize chunks (K = 1: it is all there is)
constexpr uint32_t dec2_shared_dwords(uint32_t W, uint32_t K) { return (K == 1 ? 0u : (K == 4 ? 2u : 1u) << W) + kDtab / 4; }
// decoder staging per wave: whole 16-byte-per-lane vectors (1 KiB each) covering NR * 64 words
constexpr uint32_t dec2_stage_dwords(uint32_t NR) { return ((NR + 3) / 4) * 256; }
constexpr uint32_t kRebinRowDwords = 256 + 64;  // k_decode_rebin's row buffer per wave: 1024 byte prefixes + 64 lane prefixes

// output bits per symbol of mh_decode_packed: 2 while every symbol fits (S <= 4), else 4
inline uint32_t packed_out_bits(uint32_t S) { return S <= 4 ? 2u : 4u; }
// lane-private LDS staging of the encoder: 16 dwords per lane for codes of at most 2 bits (the worst case of a
// 256-sample sub-stream), else 32 (= 4 bits per sample on average: the worst case up to 4-bit codes; a clipped
// spike-count channel at S <= 10 stays well below that, and chunks that outgrow it take the two-pass global slow
// path).  Always 4 * stage_ne(LC) rows: the staging rows are permuted so that the merge gathers consecutive dwords
// (MH_STAGE_AT), which needs the row count the kernel class was compiled for.
inline uint32_t enc_stage_dw(uint32_t maxlen) { return maxlen <= 2 ? 16 : 32; }
// Index bits W of the decode table (PlanHost::W), K symbols per lookup.  maxlen <= 5: W = K * maxlen (<= 10), every
// entry holds K whole codewords; longer codes (and W capped below 2 * maxlen): hybrid pair table of 10 index bits and 31
// staging registers, which keeps 4 workgroups per CU (tables + staging <= 40 KiB of LDS).
inline uint32_t dec_table_bits(uint32_t maxlen, bool wave)
{
    if (maxlen <= 2) return 4 * maxlen;
    // (wave-task plans build the table once per WAVE: 256 entries instead of 1024 cost a few more flagged
    // entries but a quarter of the build and 3 KiB less LDS per wave -- 2400 x 72 000, S = 8: 66 -> 58 us)
    uint32_t cap = wave ? 8u : 10u;
    if (cap < maxlen) cap = maxlen;  // a flagged entry still holds its first codeword
    return 2 * maxlen < cap ? 2 * maxlen : cap;
}

// Template arguments <K, M, NR, RL, HY> of a rung (DUAL: k_decode2w only).  Window maintenance RL
// (decode_staged_chunk): 1 = reload, 0 = branchy top-up, 2 = select top-up; the choices are the measured best per
// variant (profiles/README.md).
struct DecRung { int K, M, NR, RL; bool HY, DUAL; };
enum DecRungId { kRungQuad, kRungPair, kRungOne, kRungHybrid, kRungPair3, kDecRungCount };
constexpr DecRung kDecRungs[kDecRungCount] = {
    {4, 4, 17, 1, false, false},  // Quad    L <= 2   four symbols per lookup; worst-case chunk = 1027 words: never oversize
    {2, 2, 32, 0, false, false},  // Pair    W >= 2L  whole pairs (L <= 5 for workgroup tasks, L <= 4 for wave tasks)
    {1, 2, 36, 2, false, true},   // One     W < 2L   one symbol per lookup, two chunks side by side; wave form only
    {2, 2, 31, 2, true, false},   // Hybrid  W < 2L   one-symbol entries flagged; workgroup form only
    {2, 2, 25, 2, false, false},  // Pair3   L == 3   whole pairs in 6 index bits
};
enum DecForm { kDecode2, kDecode2w, kDecodeRange, kDecodeRebinSat, kDecodeRebinWide };  // launch forms (k_decode_rebin<..., SAT>)
struct DecPick { DecRungId rung; DecForm form; uint32_t po; };  // po: output bits of the packed decoders (2 / 4), 0 = bytes

// Instances the library builds: every rung for byte output (PO = 0); S <= 4 has no code longer than 3 bits and S >= 5
// none shorter than 3, so PO = 2 stops at L = 3 and PO = 4 starts there.  18 k_decode2 / k_decode2w instances, four
// rungs of k_decode_range and k_decode_rebin; nothing else is built.
constexpr bool dec_built(int rung, DecForm form, uint32_t po)
{
    if (po == 2 ? rung != kRungQuad && rung != kRungPair3 : po == 4 ? rung == kRungQuad : po != 0) return false;
    if (form == kDecode2w) return rung != kRungHybrid;
    return rung != kRungOne && (form == kDecode2 || po == 0);
}

// The decoder from maxlen L, the table width W and the task form; po = 0 for mh_decode, packed_out_bits(S) for
// mh_decode_packed.  The range and re-bin kernels run on the rung of the workgroup form at po = 0 (a long range on long channels
// is what matters; plans of the wave-only one-symbol rung take the hybrid pair table as long-channel plans do).
inline DecPick dec_pick(uint32_t L, uint32_t W, bool wave, uint32_t po)
{
    const DecForm form = wave ? kDecode2w : kDecode2;
    if (po != 4 && L <= 2) return {kRungQuad, form, po};
    if (po == 2 || L == 3) return {kRungPair3, form, po};
    if (W >= 2 * L) return {kRungPair, form, po};
    // Long codes on SHORT channels (wave tasks, where every wave builds its own tables): the one-symbol decoder
    // -- a 2^maxlen-byte table instead of a 256-entry hybrid pair table whose flagged entries make almost every
    // lookup of the wave take the slow path (8 index bits) -- with the two chunks of a segment side by side
    // (decode_staged_pair1).  10 000 x 20 000: decode S=8 82 -> 74 us, S=10 92 -> 77 us; 2400 x 72 000: 70 -> 68 us.
    // On long channels (shared 1024-entry tables) it loses: S=8 2.35 -> 2.82 ms -- twice the LDS lookups, and
    // those decoders are bound by LDS bank-conflict throughput, not by the latency of the chain
    // (profiles/r03_k1_pair_decoding_ab.txt).
    if (wave) return {kRungOne, form, po};
    return {kRungHybrid, form, po};
}

// Dynamic LDS of a decoder launch.  k_decode2, k_decode_range: shared tables + four waves' staging; k_decode2w: both per
// wave; k_decode_rebin: k_decode_range's plus each wave's row buffer; 64 bytes of slack behind the last wave's staging
// area, which a cut last chunk may read past by a few words (decode_staged_chunk, SINK).
inline size_t dec_lds_bytes(const DecPick &p, uint32_t W)
{
    const DecRung &r = kDecRungs[p.rung];
    const size_t tab = dec2_shared_dwords(W, (uint32_t)r.K), stage = dec2_stage_dwords((uint32_t)r.NR);
    if (p.form == kDecode2w) return 4 * (tab + stage) * sizeof(uint32_t);
    size_t lds = (tab + 4 * stage) * sizeof(uint32_t);
    if (p.form >= kDecodeRebinSat) lds += 4 * kRebinRowDwords * sizeof(uint32_t) + 64;
    // The four-symbol decoder (S <= 3) is bound by its 1-KiB row stores, not by its arithmetic, and the part
    // writes FASTER with fewer waves streaming at once: 3 workgroups per CU instead of the 4 its registers
    // allow, enforced through the LDS request (160 KiB / 41 KiB = 3): 1024 ch x 1e7 bins decode 2.25 -> 2.04 ms
    // on one box; 2 per CU: 2.40 ms (profiles/r03_occupancy_ab.txt).  The pair-table decoders (S >= 4) are
    // bound by their dependent lookup chain and lose with fewer waves (S = 5: 2.27 -> 2.38 ms).  (Measured with
    // byte output; the packed decoders request only the LDS they use.)
    if (r.K == 4 && p.po == 0 && lds < kLds3PerCu) lds = kLds3PerCu;
    return lds;
}
// LC: code class of maxlen L: <= 2, <= 4, <= 8, longer (2-bit pieces mean S <= 4, so L <= 3).  PK: input packing (0 =
// bytes, 4 / 2 = packed pieces).  PB: pair packing.  Byte input packs pairs in 3 bits while every symbol fits 3 bits
// (S <= 8; always at L <= 2), the longest class in 4 only; 4-bit pieces: a byte of the stream is the PB = 4 pair index;
// 2-bit pieces: the four-symbol table (PB unused).  wave: k_encode2w, else k_encode2.
struct EncPick { int LC, PB, PK; bool wave; };
// the instances the library builds, each in both task forms (24), in code-object order: every pick is one of them
constexpr EncPick kEncInsts[] = {{0, 4, 4, 0}, {3, 4, 4, 0}, {2, 4, 4, 0}, {1, 4, 4, 0}, {0, 4, 2, 0}, {1, 4, 2, 0},
                                 {0, 3, 0, 0}, {3, 4, 0, 0}, {2, 4, 0, 0}, {2, 3, 0, 0}, {1, 4, 0, 0}, {1, 3, 0, 0}};
inline EncPick enc_pick(uint32_t L, uint32_t S, uint32_t input_bits, bool wave)
{
    const int PK = input_bits == 8 ? 0 : (int)input_bits;
    const int LC = L <= 2 ? 0 : PK == 2 || L <= 4 ? 1 : L <= 8 ? 2 : 3;
    return {LC, PK == 0 && LC < 3 && (LC == 0 || S <= 8) ? 3 : 4, PK, wave};
}

// Dynamic LDS of an encoder launch of ntask tasks (+ the static tables of k_encode2)
inline size_t enc_lds_bytes(const EncPick &e, uint32_t maxlen, uint32_t ntask)
{
    const uint32_t dw = enc_stage_dw(maxlen);
    if (e.wave) return 4 * (size_t)(enc2w_table_dwords(e.PB, e.PK) + enc2_wave_dwords(dw)) * sizeof(uint32_t);
    size_t lds = 4 * (size_t)enc2_wave_dwords(dw) * sizeof(uint32_t);
    // The short-code byte-input encoder (S <= 3), like the S <= 3 decoder, is bound by the memory system and not by its
    // arithmetic, and runs FASTER with 3 workgroups per CU than with the 4 its registers allow: 1024 ch x 1e7 bins
    // 2.02-2.16 -> 1.975 ms with placement-probed payload buffers, and no longer sensitive to where the input sits
    // (profiles/r03_occupancy_ab.txt).  The longer-code encoders are compute-bound before their stores and lose
    // (S = 8: +4 %), S = 4..6 are indifferent (-0.8 %): only LC = 0 is capped, through the LDS request.
    // Only where the launch has many rounds of workgroups: with 2640 tasks (96 ch x 3.6e6 bins) a quarter fewer slots cost
    // a whole extra round (77.7 -> 80.2 us).
    if (e.LC == 0 && e.PK == 0 && ntask >= 16384 && lds < kLds3PerCu) lds = kLds3PerCu;
    return lds;
}

// demangled instance names, as the code object lists them (tests/planner_check.cpp)
inline std::string name_args(std::initializer_list<int> v)
{
    std::string s;
    for (int x : v) s += (s.empty() ? "<" : ", ") + std::to_string(x);
    return s;
}
inline std::string dec_name(const DecPick &p)
{
    static const char *const head[] = {"k_decode2", "k_decode2w", "k_decode_range", "k_decode_rebin", "k_decode_rebin"};
    const DecRung &r = kDecRungs[p.rung];
    const auto flag = [](bool b) { return b ? ", true" : ", false"; };
    std::string s = std::string("mh::") + head[p.form] + name_args({r.K, r.M, r.NR, r.RL}) + flag(r.HY);
    if (p.form == kDecode2w) s += flag(r.DUAL);
    if (p.form >= kDecodeRebinSat) s += flag(p.form == kDecodeRebinSat);
    return p.form <= kDecode2w ? s + ", " + std::to_string(p.po) + ">" : s + ">";
}
inline std::string enc_name(const EncPick &e) { return (e.wave ? "mh::k_encode2w" : "mh::k_encode2") + name_args({e.LC, e.PB, e.PK}) + ">"; }
}  // namespace mh
