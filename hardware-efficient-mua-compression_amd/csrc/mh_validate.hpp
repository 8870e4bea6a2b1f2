// mh_validate.hpp -- the structural walk of a STORED stream: what mh_validate_stream and mh_validate_segments do behind
// their NULL checks.  Pure C++ (no HIP, no device, no global state).  This is the part of the product that parses
// untrusted file bytes on the host -- every index it forms comes from a header word of the stream -- so it reads
// payload[i] only for i below the payload_words it was given: tests/planner_check.cpp --validate runs it under
// -fsanitize=address,undefined on payloads held in allocations of exactly that size (tests/test_host_validate.py).
// Every function returns an MH_* code and leaves the text of an error in the Msg.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "mh_msg.hpp"
#include "mh_planner.hpp"

namespace mh {

// The PlanHost of checked arguments over zero offsets (offsets do not enter the directory): what mh_plan_query reports.
inline int plan_host_of_args(Msg &m, const uint64_t *ch_len, uint32_t C, uint32_t S, uint32_t h, uint32_t mode,
                             uint32_t window, const uint8_t *sclv, uint32_t K, uint32_t seg_chunks, PlanHost &H)
{
    if (int rc = plan_args(m, ch_len, C, S, h, mode, window, sclv, K, seg_chunks, &H.info)) return rc;
    const std::vector<uint64_t> off(C, 0);
    plan_host_build(H, off.data(), ch_len, sclv);
    return MH_OK;
}

// ... and what a stored stream is walked against: it names its seg_chunks, and its directory has the layout's size.
// `who` names the validating call.
inline int stored_plan_host(Msg &m, const char *who, const uint64_t *ch_len, uint32_t C, uint32_t S, uint32_t h,
                            uint32_t mode, uint32_t window, const uint8_t *sclv, uint32_t K, uint32_t seg_chunks,
                            uint64_t n_segments, PlanHost &H)
{
    if (seg_chunks == 0) return m.set(MH_ERR_ARG, "%s: a stored stream names its seg_chunks", who);
    if (int rc = plan_host_of_args(m, ch_len, C, S, h, mode, window, sclv, K, seg_chunks, H)) return rc;
    if (H.seg_ch.size() != n_segments)
        return m.set(MH_ERR_STREAM, "directory has %llu segments, the layout implies %zu", (unsigned long long)n_segments,
                     H.seg_ch.size());
    return MH_OK;
}

// the (peak, encoder) word of channel c names a symbol and an SCLV row of the plan
inline int validate_channel_word(Msg &m, const PlanHost &H, uint32_t c, const uint8_t *peak, const uint8_t *enc)
{
    const uint32_t S = H.info.S, K = H.info.K;
    if (peak[c] >= S || enc[c] >= K)
        return m.set(MH_ERR_STREAM, "channel %u: (peak %u, encoder %u) outside (S=%u, K=%u)", c, peak[c], enc[c], S, K);
    return MH_OK;
}

// The stored segment s (directory entry of H) in payload[pos, pos + words): inside the payload_words there are, then its
// chunk walk -- header sizes, sub-stream lengths possible for the channel's code, chunk sizes adding up exactly to its
// end.  enc[channel] is already checked (validate_channel_word).  The limits are subtractive: no offset wraps them.
inline int validate_segment(Msg &m, const PlanHost &H, uint64_t s, const uint32_t *payload, uint64_t payload_words,
                            uint64_t pos, uint64_t words, const uint8_t *enc)
{
    if (pos > payload_words || words > payload_words - pos)
        return m.set(MH_ERR_STREAM, "segment %llu ends at word %llu, the payload has %llu", (unsigned long long)s,
                     (unsigned long long)(pos + words), (unsigned long long)payload_words);
    const uint32_t S = H.info.S;
    const uint64_t end = pos + words;
    const uint64_t maxlen = H.sclv[(size_t)enc[H.seg_ch[s]] * S + S - 1];  // the row is sorted: its longest codeword
    uint64_t left = H.seg_n[s];
    while (left) {
        const uint64_t chunk_n = left < MH_CHUNK ? left : MH_CHUNK;
        if (pos >= end) return m.set(MH_ERR_STREAM, "segment %llu is shorter than its chunk headers say", (unsigned long long)s);
        const uint32_t w0 = payload[pos];
        const uint32_t mn = w0 & 0xFFFu, w = (w0 >> 12) & 15u;
        if (w > 12) return m.set(MH_ERR_STREAM, "segment %llu: chunk header field width %u above 12", (unsigned long long)s, w);
        const uint64_t hw = (16u + 64u * w + 31u) >> 5;
        if (hw > end - pos) return m.set(MH_ERR_STREAM, "segment %llu: chunk header runs past the segment", (unsigned long long)s);
        uint64_t sum = 0, longest = 0;
        for (uint32_t l = 0; l < 64; ++l) {
            uint64_t f = 0;
            if (w) {
                const uint32_t fb = 16u + l * w;
                uint64_t v = payload[pos + (fb >> 5)];
                if ((fb & 31) + w > 32) v |= (uint64_t)payload[pos + (fb >> 5) + 1] << 32;
                f = (v >> (fb & 31)) & ((1u << w) - 1u);
            }
            sum += mn + f;
            if (mn + f > longest) longest = mn + f;
        }
        // every codeword has 1..maxlen bits; a sub-stream holds <= 256 samples
        if (longest > 256 * maxlen || sum > chunk_n * maxlen || sum < chunk_n)
            return m.set(MH_ERR_STREAM, "segment %llu: sub-stream lengths impossible for this code", (unsigned long long)s);
        pos += hw + ((sum + 31) >> 5);  // (at most 25 + 4608 words: past `end`, never around)
        left -= chunk_n;
    }
    if (pos != end)
        return m.set(MH_ERR_STREAM, "segment %llu: chunk sizes do not add up to its %llu words", (unsigned long long)s,
                     (unsigned long long)words);
    return MH_OK;
}

// The whole stream: every channel's word, the segments back to back from word 0, nothing behind the last one.
// seg_words has H.seg_ch.size() entries (stored_plan_host compared the counts).
inline int validate_stream(Msg &m, const PlanHost &H, const uint32_t *payload, uint64_t payload_words,
                           const uint64_t *seg_words, const uint8_t *peak, const uint8_t *enc)
{
    for (uint32_t c = 0; c < H.info.C; ++c)
        if (int rc = validate_channel_word(m, H, c, peak, enc)) return rc;
    uint64_t pos = 0;
    for (size_t s = 0; s < H.seg_ch.size(); ++s) {
        if (int rc = validate_segment(m, H, s, payload, payload_words, pos, seg_words[s], enc)) return rc;
        pos += seg_words[s];
    }
    if (pos != payload_words)
        return m.set(MH_ERR_STREAM, "payload has %llu words, the directory accounts for %llu", (unsigned long long)payload_words,
                     (unsigned long long)pos);
    return MH_OK;
}

// The listed segments only (what a range query reads), each where seg_off puts it; `who` names the call.
inline int validate_segments(Msg &m, const char *who, const PlanHost &H, const uint32_t *payload, uint64_t payload_words,
                             const uint64_t *seg_off, const uint64_t *seg_words, const uint64_t *seg_idx, uint64_t n_idx,
                             const uint8_t *peak, const uint8_t *enc)
{
    const uint64_t n_segments = H.seg_ch.size();
    for (uint64_t j = 0; j < n_idx; ++j) {
        const uint64_t s = seg_idx[j];
        if (s >= n_segments)
            return m.set(MH_ERR_ARG, "%s: seg_idx[%llu] = %llu, the directory has %llu entries", who, (unsigned long long)j,
                         (unsigned long long)s, (unsigned long long)n_segments);
        if (int rc = validate_channel_word(m, H, H.seg_ch[s], peak, enc)) return rc;
        if (int rc = validate_segment(m, H, s, payload, payload_words, seg_off[s], seg_words[s], enc)) return rc;
    }
    return MH_OK;
}

}  // namespace mh
