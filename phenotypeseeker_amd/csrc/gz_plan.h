// The host's part of the device inflate (gz_inflate.hip, step 3 of its header comment) as plain functions over the files' bytes
// and the numbers a counting pass returns: the cut into chunks, the candidate starts, the walk along the links, the rule that
// a chain is whole members, the layout of the text.  This is what decides whether a file of untrusted bytes is trusted or
// handed to zlib.  Nothing here touches the device, a context or the environment (knob values arrive as arguments), so it can
// be compiled and checked on its own: tests/gz_plan_check.cpp plays the device's part with zlib.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <tuple>
#include <utility>
#include <vector>

// (seen by the kernels of gz_inflate.hip as well)
constexpr uint64_t GZ_NONE = ~0ull;
constexpr int GZ_FINAL = -1, GZ_ERROR = -2, GZ_OVERRUN = -3, GZ_STOP = -5;
constexpr int GZ_WIN = 32768;

struct GzMemberHead {
    size_t deflate_at = 0;   // offset of the DEFLATE data in the file
    uint32_t bsize = 0;      // BGZF: length of the whole member (0: not a BGZF member)
};

// RFC 1952 2.3; false: no gzip member starts at `at`
inline bool gz_parse_member_header(const uint8_t *d, size_t n, size_t at, GzMemberHead *h)
{
    if (at + 18 > n || d[at] != 0x1f || d[at + 1] != 0x8b || d[at + 2] != 8) return false;
    const uint8_t flg = d[at + 3];
    if (flg & 0xe0) return false;
    size_t p = at + 10;
    h->bsize = 0;
    if (flg & 4) {
        if (p + 2 > n) return false;
        const size_t xlen = d[p] | (d[p + 1] << 8);
        p += 2;
        if (p + xlen > n) return false;
        for (size_t q = p; q + 4 <= p + xlen;) {
            const size_t sl = d[q + 2] | (d[q + 3] << 8);
            if (d[q] == 'B' && d[q + 1] == 'C' && sl == 2 && q + 6 <= p + xlen) h->bsize = (uint32_t)(d[q + 4] | (d[q + 5] << 8)) + 1;
            q += 4 + sl;
        }
        p += xlen;
    }
    if (flg & 8) {
        while (p < n && d[p]) p++;
        p++;
    }
    if (flg & 16) {
        while (p < n && d[p]) p++;
        p++;
    }
    if (flg & 2) p += 2;
    if (p + 8 > n) return false;
    h->deflate_at = p;
    return true;
}

inline uint32_t gz_le32(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }

struct GzChunk {
    int file;
    uint64_t start_bit;   // in the device image (GZ_NONE until found)
    uint64_t seek_from, seek_to;   // bits: where gz_find_kernel looks (seek_from == seek_to: the start is known)
    bool true_start;
    // results of the counting pass
    uint64_t out_len = 0, n_rec = 0, end_bit = 0;
    int32_t link = GZ_ERROR;
    bool counted = false;
};

struct GzFile {
    const uint8_t *data;
    size_t size;
    uint64_t at;          // offset of the image in the device buffer
    bool bgzf = false;
    bool device_ok = true;
    std::vector<int> chain;      // its chunks in stream order
    uint64_t out_off = 0, out_len = 0;
    int nul_slot = -1;    // its entry of the writing pass's per-file tables
};

// Where the images of a group lie in its device buffer (16-byte aligned, at least 16 zero bytes behind each); returns its size.
inline uint64_t gz_image_layout(int n, const size_t *sizes, uint64_t *at)
{
    uint64_t total = 0;
    for (int i = 0; i < n; i++) {
        at[i] = total;
        total += (sizes[i] + 16 + 15) & ~(size_t)15;
    }
    return total + 64;
}

// Bytes between two cuts: `knob` when given, else the group's bytes over the lanes wanted, 16 KB to 4 MB.  (16 KB: less than a
// block of most encoders -- two cuts in one block find the same start and one of the two lanes idles, but a group that cannot
// fill the part anyway is cut at every block: 1.15 GB of FASTQ text 69 -> 51 ms)
inline size_t gz_chunk_bytes(size_t bytes, size_t lanes, size_t knob)
{
    const size_t chunk = knob ? knob : std::min<size_t>(std::max<size_t>(bytes / lanes, 16 << 10), 4 << 20);
    return (chunk + 3) & ~(size_t)3;
}

// ---- the chunks of a group, and where every file's chain stands -----------------------------------------------------
struct GzPlan {
    std::vector<GzFile> files;
    std::vector<GzChunk> ch;
    std::vector<std::pair<int, int>> file_chunks;   // per file: [first, last) of its regular chunks
    std::vector<int> next_chunk;                    // per file: the chunk its chain follows next (-1: the chain has reached the end)
    std::vector<int> todo;                          // chunks of the coming counting pass
    uint64_t comp_total = 0;                        // bytes of the group's device image
};

// The cut.  A file whose header does not parse is declined.  BGZF: every member says how long it is -- one chunk per member,
// nothing to search for; any inconsistency declines the file.  Else a cut every `chunk` bytes from the DEFLATE data to the
// trailer: the first has its known start, the others a range to search.
inline GzPlan gz_plan_chunks(int n, const uint8_t *const *data, const size_t *sizes, size_t chunk)
{
    GzPlan p;
    p.files.resize((size_t)n);
    p.file_chunks.resize((size_t)n);
    p.next_chunk.assign((size_t)n, -1);
    std::vector<uint64_t> image_at((size_t)n);
    p.comp_total = gz_image_layout(n, sizes, image_at.data());
    for (int i = 0; i < n; i++) {
        GzFile &f = p.files[(size_t)i];
        f.data = data[i];
        f.size = sizes[i];
        f.at = image_at[(size_t)i];
        GzMemberHead h;
        p.file_chunks[(size_t)i] = {(int)p.ch.size(), (int)p.ch.size()};
        if (!gz_parse_member_header(f.data, f.size, 0, &h)) {
            f.device_ok = false;
            continue;
        }
        if (h.bsize) {
            f.bgzf = true;
            size_t at = 0;
            bool ok = true;
            while (at < f.size) {
                GzMemberHead m;
                if (!gz_parse_member_header(f.data, f.size, at, &m) || !m.bsize || at + m.bsize > f.size || m.deflate_at + 8 > at + m.bsize) {
                    ok = false;
                    break;
                }
                GzChunk c;
                c.file = i;
                c.start_bit = (f.at + m.deflate_at) * 8;
                c.seek_from = c.seek_to = 0;
                c.true_start = true;
                p.ch.push_back(c);
                at += m.bsize;
            }
            if (!ok) {
                p.ch.resize((size_t)p.file_chunks[(size_t)i].first);
                f.bgzf = false;
                f.device_ok = false;
                continue;
            }
        } else {
            const size_t d0 = h.deflate_at, d1 = f.size - 8;
            for (size_t at = d0; at < d1 || at == d0; at += chunk) {
                GzChunk c;
                c.file = i;
                c.true_start = at == d0;
                c.start_bit = at == d0 ? (f.at + d0) * 8 : GZ_NONE;
                c.seek_from = at == d0 ? 0 : (f.at + at) * 8;
                c.seek_to = at == d0 ? 0 : (f.at + std::min(at + chunk, d1)) * 8;
                p.ch.push_back(c);
            }
        }
        p.file_chunks[(size_t)i].second = (int)p.ch.size();
        if (p.file_chunks[(size_t)i].second > p.file_chunks[(size_t)i].first) p.next_chunk[(size_t)i] = p.file_chunks[(size_t)i].first;
    }
    for (size_t c = 0; c < p.ch.size(); c++) p.todo.push_back((int)c);
    return p;
}

// ---- the starts a block end may coincide with: per file, ascending ---------------------------------------------------
struct GzCands {
    std::vector<uint64_t> bit;
    std::vector<int> chunk;   // whose start bit[i] is
    std::vector<std::pair<uint32_t, uint32_t>> of_file;

    void rebuild(const GzPlan &p)
    {
        std::vector<std::tuple<int, uint64_t, int>> v;   // (file, start, chunk)
        for (size_t c = 0; c < p.ch.size(); c++)
            if (p.ch[c].start_bit != GZ_NONE) v.emplace_back(p.ch[c].file, p.ch[c].start_bit, (int)c);
        std::sort(v.begin(), v.end());
        bit.clear();
        chunk.clear();
        of_file.assign(p.files.size(), {0u, 0u});
        size_t e = 0;
        for (size_t i = 0; i < p.files.size(); i++) {
            of_file[i].first = (uint32_t)bit.size();
            for (; e < v.size() && std::get<0>(v[e]) == (int)i; e++) {
                bit.push_back(std::get<1>(v[e]));
                chunk.push_back(std::get<2>(v[e]));
            }
            of_file[i].second = (uint32_t)bit.size();
        }
    }
    // [from, to) of `bit` for a chunk: the starts of its file behind its own (a chunk without a start: none)
    std::pair<uint32_t, uint32_t> range(const GzChunk &c) const
    {
        const auto &fc = of_file[(size_t)c.file];
        if (c.start_bit == GZ_NONE) return {fc.second, fc.second};
        return {(uint32_t)(std::upper_bound(bit.begin() + fc.first, bit.begin() + fc.second, c.start_bit) - bit.begin()), fc.second};
    }
};

// ---- a counting round's results, and the walk along the links ---------------------------------------------------------
// entry j of the four arrays: what the pass returned for chunk todo[j] (link: an entry of cands.bit, or negative)
inline void gz_apply_round(GzPlan &p, const GzCands &cands, const uint64_t *out_len, const uint64_t *n_rec, const uint64_t *end_bit, const int32_t *link)
{
    for (size_t j = 0; j < p.todo.size(); j++) {
        GzChunk &c = p.ch[(size_t)p.todo[j]];
        if (c.start_bit == GZ_NONE || !p.files[(size_t)c.file].device_ok) continue;
        c.counted = true;
        c.out_len = out_len[j];
        c.n_rec = n_rec[j];
        c.end_bit = end_bit[j];
        c.link = link[j] >= 0 ? cands.chunk[(size_t)link[j]] : link[j];
    }
}

// Every file's chain as far as the counted chunks carry it; p.todo becomes what the next round has to count (a member in the
// middle of a file that no found start coincides with: one more chunk).
inline void gz_walk_chains(GzPlan &p)
{
    std::vector<GzChunk> &ch = p.ch;
    p.todo.clear();
    for (size_t i = 0; i < p.files.size(); i++) {
        GzFile &f = p.files[i];
        int &next_chunk = p.next_chunk[i];
        while (f.device_ok && next_chunk >= 0) {
            const int cidx = next_chunk;
            GzChunk &c = ch[(size_t)cidx];
            if (!c.counted) break;   // in `todo`: the next round
            f.chain.push_back(cidx);
            if (c.link >= 0) {
                if (ch[(size_t)c.link].true_start) {
                    // a block that ends, without being the last of its member, where another member's data begin: no
                    // stream zlib accepts does that (a crafted BSIZE / member header does): zlib words the error
                    f.device_ok = false;
                    break;
                }
                next_chunk = c.link;
                continue;
            }
            if (c.link != GZ_FINAL) {
                f.device_ok = false;   // an error, or a block that ran on and on: zlib decides what it is
                break;
            }
            // the member's trailer; another member behind it?
            const uint64_t trailer = (c.end_bit + 7) / 8 - f.at;
            if (trailer + 8 > f.size) {
                f.device_ok = false;
                break;
            }
            size_t next = (size_t)trailer + 8;
            {
                // ISIZE of the member that just ended: the bytes since its true start
                uint64_t member = 0;
                for (size_t q = f.chain.size(); q-- > 0;) {
                    member += ch[(size_t)f.chain[q]].out_len;
                    if (ch[(size_t)f.chain[q]].true_start) break;
                }
                if ((uint32_t)member != gz_le32(f.data + trailer + 4)) {
                    f.device_ok = false;
                    break;
                }
            }
            while (next < f.size && f.data[next] == 0) next++;   // padding (gzip.decompress skips it as well)
            if (next >= f.size) {
                next_chunk = -1;
                break;
            }
            if (f.bgzf) {
                // the next member is the next chunk of the file
                next_chunk = cidx + 1 < p.file_chunks[i].second ? cidx + 1 : -1;
                if (next_chunk < 0) f.device_ok = false;
                continue;
            }
            GzMemberHead h;
            if (!gz_parse_member_header(f.data, f.size, next, &h)) {
                f.device_ok = false;
                break;
            }
            // a member in the middle of the file: it starts a chain of its own (a chunk whose found start this is
            // becomes its first link; else one more chunk, counted in the next round)
            const uint64_t sbit = (f.at + h.deflate_at) * 8;
            int have = -1;
            for (int q = p.file_chunks[i].first; q < (int)ch.size(); q++)
                if (ch[(size_t)q].file == (int)i && ch[(size_t)q].start_bit == sbit) have = q;
            if (have >= 0) {
                ch[(size_t)have].true_start = true;   // (what it counted stays right: a valid stream has no match reaching back here)
                next_chunk = have;
                continue;
            }
            GzChunk extra;
            extra.file = (int)i;
            extra.start_bit = sbit;
            extra.seek_from = extra.seek_to = 0;
            extra.true_start = true;
            ch.push_back(extra);
            p.todo.push_back((int)ch.size() - 1);
            next_chunk = (int)ch.size() - 1;
            break;
        }
    }
}

// the rounds have run out: a file with a chunk still to count is declined
inline void gz_decline_unfinished(GzPlan &p)
{
    for (int c : p.todo) p.files[(size_t)p.ch[(size_t)c].file].device_ok = false;
}

// A file's chain is members one after the other -- first chunk a member's start, none in the middle of a member (a chunk
// that was linked to BEFORE a later walk found a member starting there), the last chunk the end of a member: anything else
// is declined here, so that every member of the layout has a beginning AND a length and the check sums are never skipped
inline void gz_keep_whole_members(GzPlan &p)
{
    for (GzFile &f : p.files) {
        if (!f.device_ok) continue;
        bool open = false, ok = !f.chain.empty();
        for (int c : f.chain) {
            const GzChunk &k = p.ch[(size_t)c];
            if (k.true_start == open) ok = false;   // a start inside a member, or a member that does not begin with one
            open = k.link != GZ_FINAL;
        }
        if (!ok || open) f.device_ok = false;
    }
}

// ---- the layout of the text -------------------------------------------------------------------------------------------
struct GzTextLayout {
    uint64_t total = GZ_WIN;   // (room before the first file: a marker of a corrupt stream reads inside the buffer)
    uint64_t total_rec = 0;
    std::vector<int> order;    // the chunks of the writing pass, file by file, in stream order
    std::vector<uint32_t> file_first;   // per file of the pass, and one more: its first entry of `order`
    std::vector<uint8_t> members_only;  // per file of the pass: every chunk a member's start (no window to resolve)
    std::vector<uint64_t> c_off, c_rec; // per entry of `order`: where its text and its matches go
    std::vector<uint64_t> m_begin, m_len;   // the members, in the order of the text buffer
    std::vector<uint32_t> m_crc;            // ... what their trailers say
    std::vector<int> m_file;
    bool members_whole() const { return m_begin.size() == m_len.size() && m_len.size() == m_crc.size(); }
};

// Every accepted file's text starts at a multiple of 64; its out_off / out_len / nul_slot are set here.
inline GzTextLayout gz_layout_text(GzPlan &p)
{
    GzTextLayout L;
    for (size_t i = 0; i < p.files.size(); i++) {
        GzFile &f = p.files[i];
        if (!f.device_ok) continue;
        L.total = (L.total + 63) & ~63ull;
        f.out_off = L.total;
        f.nul_slot = (int)L.file_first.size();
        L.file_first.push_back((uint32_t)L.order.size());
        bool members_only = true;
        for (int c : f.chain) {
            const GzChunk &k = p.ch[(size_t)c];
            L.order.push_back(c);
            L.c_off.push_back(L.total);
            if (k.true_start) L.m_begin.push_back(L.total);
            members_only = members_only && k.true_start;
            L.total += k.out_len;
            L.c_rec.push_back(L.total_rec);
            L.total_rec += k.n_rec;
            if (k.link == GZ_FINAL) {   // the member's trailer: CRC-32, ISIZE
                L.m_len.push_back(L.total - L.m_begin.back());
                L.m_crc.push_back(gz_le32(f.data + ((k.end_bit + 7) / 8 - f.at)));
                L.m_file.push_back((int)i);
            }
        }
        L.members_only.push_back(members_only ? 1 : 0);
        f.out_len = L.total - f.out_off;
    }
    L.file_first.push_back((uint32_t)L.order.size());
    L.total = (L.total + 63) & ~63ull;
    return L;
}
