// georec.h — the host side of the GeoIP ANSWER tables (PWAF_OPT_GEO_ANSWERS): the flattening of the record-leaf GeoIP trie
// (Program::geo_trie) into the 2^24-entry IPv4 table that dirtable::compress takes, and a scalar restatement of georec_kernel's
// lookup. pwaf_engine_create and the CPU suite (tests/georec_host.cpp) compile this very header.
//
// The class tables of ipres_kernel (dirtable.h) say which PREDICATES hold for an address; these say which RECORD it has — what the
// reference puts into its RequestContext and sends upstream (http_listener.rs:143-157,183-191; http_proxy_service.rs:174-189).
// One table entry per /24: the record id when the trie ends within 24 bits, else kEscape | the index of the 8-bit trie node the
// lookup continues from with the address's last byte (an IPv4 trie is 16 + 8 + 8 bits deep, so that node's entries are leaves;
// the node index itself is the payload: no side table). Record ids and node indices are below 2^31.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "dirtable.h"

namespace pwaf {
namespace georec {

static constexpr uint32_t kLeaf = 0x80000000u;    // program.h: TRIE_LEAF
static constexpr uint32_t kEscape = 0x80000000u;  // table entry: continue in trie node (entry & ~kEscape)

// root4: 65536 entries (leaf | record, or a node index); nodes: 256 entries each. -> d24 (2^24 entries); returns the escaped /24s.
inline uint32_t flatten(const uint32_t *root4, const uint32_t *nodes, std::vector<uint32_t> &d24) {
    d24.resize(dirtable::kEntries);
    uint32_t n_esc = 0;
    for (uint32_t t = 0; t < 65536u; t++) {
        const uint32_t e = root4[t];
        uint32_t *dst = &d24[(size_t)t << 8];
        if (e & kLeaf) {
            for (uint32_t b = 0; b < 256u; b++) dst[b] = e & ~kLeaf;
            continue;
        }
        const uint32_t *nd = &nodes[(size_t)e * 256];
        for (uint32_t b = 0; b < 256u; b++) {
            if (nd[b] & kLeaf) dst[b] = nd[b] & ~kLeaf;
            else { dst[b] = kEscape | nd[b]; n_esc++; }
        }
    }
    return n_esc;
}

// GeoipDB::lookup, pingoo/geoip.rs:73-91: loopback and multicast addresses are "not found"
inline bool excluded(const uint8_t ip[16], bool v6) {
    if (!v6) return ip[0] == 127u || (ip[0] & 0xF0u) == 0xE0u;
    bool loopback = ip[15] == 1;
    for (int j = 0; j < 15; j++) loopback = loopback && ip[j] == 0;
    return loopback || ip[0] == 0xFFu;
}

// What the device holds. A family without prefixes has a null root (the engine uploads an all-leaf one: record 0).
struct View {
    bool has_geo = false;
    const uint32_t *root4 = nullptr, *root6 = nullptr, *nodes = nullptr;
    size_t n_nodes = 0;
    const dirtable::Compressed *dir = nullptr;  // the IPv4 table; null: IPv4 addresses walk the trie from root4
    uint64_t out_of_range = 0;                  // (the harness asserts that no index left its table)
};

// phases 1b - 2 of the kernel: summary bit -> 16-byte record -> rank -> carried / first / further run
inline uint32_t table_entry(View &V, uint32_t x /* top 24 bits */) {
    const dirtable::Compressed &C = *V.dir;
    if (!C.summary.empty()) {
        const uint32_t blk = x >> C.shift;
        if (!((C.summary[blk >> 5] >> (blk & 31u)) & 1u)) return C.common;
    }
    const uint32_t b2 = x & 0xFFu;
    const uint32_t *rec = &C.chunks[(size_t)(x >> 8) * dirtable::kChunkWords + 4u * (b2 >> 5)];
    const uint32_t rank = (uint32_t)__builtin_popcount(rec[0] & (0xFFFFFFFFu >> (31u - (b2 & 31u))));
    if (rank == 0) return rec[1];
    if (rank == 1) return rec[2];
    const size_t at = (size_t)rec[3] + rank - 2u;
    if (at >= C.vals.size()) { V.out_of_range++; return 0; }
    return C.vals[at];
}

// -> record id (0 = the default {0, "XX"})
inline uint32_t lookup(View &V, const uint8_t ip[16], bool v6) {
    if (!V.has_geo || excluded(ip, v6)) return 0;
    uint32_t e, k;
    if (!v6 && V.dir) {
        const uint32_t t = table_entry(V, (uint32_t)ip[0] << 16 | (uint32_t)ip[1] << 8 | ip[2]);
        if (!(t & kEscape)) return t;
        e = t & ~kEscape;
        k = 3;
    } else {
        const uint32_t *root = v6 ? V.root6 : V.root4;
        if (!root) return 0;
        e = root[(uint32_t)ip[0] << 8 | ip[1]];
        k = 2;
    }
    while (!(e & kLeaf)) {
        if (e >= V.n_nodes) { V.out_of_range++; return 0; }
        e = V.nodes[(size_t)e * 256 + ip[k < 16 ? k : 15u]];
        k++;
    }
    return e & ~kLeaf;
}

}  // namespace georec
}  // namespace pwaf
