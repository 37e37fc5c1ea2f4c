// tkmk_transcript.hpp — the part of the protocol glue that needs no device: the Fiat-Shamir transcript and the Solidity-verifier
// formatting, the compiled-language mirror of the reference's Rust for
//   RollingKeccakTranscript / TranscriptManager   prove/src/lib.rs:3211-3731 (byte layout fixed by the Solidity verifier)
//   split_g1 / scalar_to_hex / split_push! / pop_recover!   libs/src/iotools/mod.rs:1625-1700
// Split out of tkmk_protocol.hpp (which includes it) so that the verifier (host/tkmk_verify.hpp, bin/verify) can replay a transcript and
// read proof.json / preprocess.json without libtkmk_hip.so.  Header-only; uses include/tkmk.h for its record types alone.
#pragma once
#include <array>
#include <iterator>
#include <string>
#include <vector>

#include "tkmk_base.hpp"

namespace tkmk {

// ---------------------------------------------------------------------------------------------------------------------
// Keccak-256 (original padding 0x01) — the hash of the transcript
// ---------------------------------------------------------------------------------------------------------------------
inline std::array<uint8_t, 32> keccak256(const uint8_t *data, size_t len) {
    static const uint64_t RC[24] = {0x0000000000000001ull, 0x0000000000008082ull, 0x800000000000808Aull, 0x8000000080008000ull,
                                    0x000000000000808Bull, 0x0000000080000001ull, 0x8000000080008081ull, 0x8000000000008009ull,
                                    0x000000000000008Aull, 0x0000000000000088ull, 0x0000000080008009ull, 0x000000008000000Aull,
                                    0x000000008000808Bull, 0x800000000000008Bull, 0x8000000000008089ull, 0x8000000000008003ull,
                                    0x8000000000008002ull, 0x8000000000000080ull, 0x000000000000800Aull, 0x800000008000000Aull,
                                    0x8000000080008081ull, 0x8000000000008080ull, 0x0000000080000001ull, 0x8000000080008008ull};
    static const int ROT[5][5] = {{0, 36, 3, 41, 18}, {1, 44, 10, 45, 2}, {62, 6, 43, 15, 61}, {28, 55, 25, 21, 56}, {27, 20, 39, 8, 14}};
    auto rol = [](uint64_t x, int n) { return n ? (x << n) | (x >> (64 - n)) : x; };
    const size_t rate = 136;
    std::vector<uint8_t> msg(data, data + len);
    msg.push_back(0x01);
    while (msg.size() % rate) msg.push_back(0);
    msg.back() |= 0x80;
    uint64_t a[5][5] = {};
    for (size_t off = 0; off < msg.size(); off += rate) {
        for (size_t i = 0; i < rate / 8; i++) {
            uint64_t w = 0;
            for (int b = 7; b >= 0; b--) w = (w << 8) | msg[off + 8 * i + b];
            a[i % 5][i / 5] ^= w;
        }
        for (int round = 0; round < 24; round++) {
            uint64_t c[5], d[5], b[5][5];
            for (int x = 0; x < 5; x++) c[x] = a[x][0] ^ a[x][1] ^ a[x][2] ^ a[x][3] ^ a[x][4];
            for (int x = 0; x < 5; x++) d[x] = c[(x + 4) % 5] ^ rol(c[(x + 1) % 5], 1);
            for (int x = 0; x < 5; x++)
                for (int y = 0; y < 5; y++) a[x][y] ^= d[x];
            for (int x = 0; x < 5; x++)
                for (int y = 0; y < 5; y++) b[y][(2 * x + 3 * y) % 5] = rol(a[x][y], ROT[x][y]);
            for (int x = 0; x < 5; x++)
                for (int y = 0; y < 5; y++) a[x][y] = b[x][y] ^ (~b[(x + 1) % 5][y] & b[(x + 2) % 5][y]);
            a[0][0] ^= RC[round];
        }
    }
    std::array<uint8_t, 32> out{};
    for (int i = 0; i < 4; i++)
        for (int b = 0; b < 8; b++) out[8 * i + b] = (uint8_t)(a[i % 5][i / 5] >> (8 * b));
    return out;
}

// big-endian bytes of a little-endian limb struct (Fr: 32, Fq: 48)
template <class T>
inline std::vector<uint8_t> be_bytes(const T &v) {
    const uint8_t *p = reinterpret_cast<const uint8_t *>(&v);
    return std::vector<uint8_t>(std::reverse_iterator<const uint8_t *>(p + sizeof(T)), std::reverse_iterator<const uint8_t *>(p));
}

// prove/src/lib.rs:3211-3400
class RollingKeccakTranscript {
  public:
    std::array<uint8_t, 32> state_0{}, state_1{};
    uint32_t challenge_counter = 0;

    void update(const uint8_t *bytes, size_t len) {
        if (len > 32) throw Error("Input must be 32 bytes or less");
        uint8_t buf[100] = {};
        std::memcpy(buf + 4, state_0.data(), 32);
        std::memcpy(buf + 36, state_1.data(), 32);
        std::memcpy(buf + 100 - len, bytes, len);   // right-aligned in the last 32-byte slot
        buf[3] = 0;
        auto s0 = keccak256(buf, 100);
        buf[3] = 1;
        auto s1 = keccak256(buf, 100);               // both from the OLD state pair
        state_0 = s0;
        state_1 = s1;
    }
    std::array<uint8_t, 32> get_challenge_raw() {
        uint8_t buf[72] = {};
        buf[3] = 2;
        std::memcpy(buf + 4, state_0.data(), 32);
        std::memcpy(buf + 36, state_1.data(), 32);
        buf[68] = (uint8_t)(challenge_counter >> 24);
        buf[69] = (uint8_t)(challenge_counter >> 16);
        buf[70] = (uint8_t)(challenge_counter >> 8);
        buf[71] = (uint8_t)challenge_counter;
        challenge_counter++;
        return keccak256(buf, 72);
    }
    // FR_MASK: top 3 bits of the big-endian hash cleared; zero -> one (:3363-3394)
    ScalarField get_challenge() {
        auto raw = get_challenge_raw();
        raw[0] &= 0x1f;
        ScalarField s{};
        uint8_t *p = reinterpret_cast<uint8_t *>(&s);
        for (int i = 0; i < 32; i++) p[i] = raw[31 - i];
        if (fr_is_zero(s)) return fr_from_u32(1);
        return s;
    }
    std::vector<ScalarField> get_challenges(size_t count) {
        std::vector<ScalarField> out;
        for (size_t i = 0; i < count; i++) out.push_back(get_challenge());
        return out;
    }
    void commit_field_as_bytes(const ScalarField &s) {       // :3416-3426
        auto be = be_bytes(s);
        update(be.data(), 32);
    }
    void commit_bls12_381_field_element(const tkmk_fq &v) {  // :3429-3480
        auto be = be_bytes(v);
        uint8_t part1[32] = {};
        std::memcpy(part1 + 16, be.data(), 16);
        update(part1, 32);
        update(be.data() + 16, 32);
    }
    void commit_g1_point(const G1Affine &p) {                // :3482-3500
        commit_bls12_381_field_element(p.x);
        commit_bls12_381_field_element(p.y);
    }
};

// commit order of the rounds (prove/src/lib.rs:3528-3731)
class TranscriptManager {
  public:
    RollingKeccakTranscript transcript;
    void add_proof0(const G1Affine &U, const G1Affine &V, const G1Affine &W, const G1Affine &Q_AX, const G1Affine &Q_AY, const G1Affine &B) {
        for (const G1Affine *p : {&U, &V, &W, &Q_AX, &Q_AY, &B}) transcript.commit_g1_point(*p);
    }
    std::vector<ScalarField> get_thetas() { return transcript.get_challenges(3); }
    void add_proof1(const G1Affine &R) { transcript.commit_g1_point(R); }
    ScalarField get_kappa0() { return transcript.get_challenge(); }
    void add_proof2(const G1Affine &Q_CX, const G1Affine &Q_CY) {
        transcript.commit_g1_point(Q_CX);
        transcript.commit_g1_point(Q_CY);
    }
    std::pair<ScalarField, ScalarField> get_chi_zeta() {
        ScalarField chi = transcript.get_challenge();
        ScalarField zeta = transcript.get_challenge();
        return {chi, zeta};
    }
    void add_proof3(const ScalarField &V_eval, const ScalarField &R_eval, const ScalarField &R_omegaX_eval, const ScalarField &R_omegaX_omegaY_eval) {
        for (const ScalarField *s : {&V_eval, &R_eval, &R_omegaX_eval, &R_omegaX_omegaY_eval}) transcript.commit_field_as_bytes(*s);
    }
    ScalarField get_kappa1() { return transcript.get_challenge(); }
};

// ---------------------------------------------------------------------------------------------------------------------
// Solidity-verifier formatting (libs/src/iotools/mod.rs:1625-1700)
// ---------------------------------------------------------------------------------------------------------------------
inline std::string hex0x(const uint8_t *p, size_t n) {
    static const char *d = "0123456789abcdef";
    std::string s = "0x";
    for (size_t i = 0; i < n; i++) {
        s.push_back(d[p[i] >> 4]);
        s.push_back(d[p[i] & 15]);
    }
    return s;
}
// -> x_part1, x_part2, y_part1, y_part2
inline std::array<std::string, 4> split_g1(const G1Affine &p) {
    auto x = be_bytes(p.x), y = be_bytes(p.y);
    return {hex0x(x.data(), 16), hex0x(x.data() + 16, 32), hex0x(y.data(), 16), hex0x(y.data() + 16, 32)};
}
inline std::string scalar_to_hex(const ScalarField &s) {
    auto be = be_bytes(s);
    return hex0x(be.data(), 32);
}
inline std::vector<uint8_t> unhex(const std::string &h) {
    size_t off = h.rfind("0x", 0) == 0 ? 2 : 0;
    if ((h.size() - off) % 2) throw Error("Invalid format");
    std::vector<uint8_t> out;
    auto nib = [](char c) -> int { return c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : c >= 'A' && c <= 'F' ? c - 'A' + 10 : -1; };
    for (size_t i = off; i < h.size(); i += 2) {
        int a = nib(h[i]), b = nib(h[i + 1]);
        if (a < 0 || b < 0) throw Error("Invalid format");
        out.push_back((uint8_t)(a * 16 + b));
    }
    return out;
}
inline tkmk_fq recover_basefield(const std::string &part1, const std::string &part2) {   // :1675-1685
    auto a = unhex(part1), b = unhex(part2);
    if (a.size() != 16 || b.size() != 32) throw Error("Invalid format");
    uint8_t be[48];
    std::memcpy(be, a.data(), 16);
    std::memcpy(be + 16, b.data(), 32);
    tkmk_fq v{};
    uint8_t *p = reinterpret_cast<uint8_t *>(&v);
    for (int i = 0; i < 48; i++) p[i] = be[47 - i];
    return v;
}
struct FormattedEntries {
    std::vector<std::string> part1, part2;
};
inline void split_push(FormattedEntries &f, const G1Affine &p) {   // split_push! (:1660-1673)
    auto s = split_g1(p);
    f.part1.push_back(s[0]);
    f.part2.push_back(s[1]);
    f.part1.push_back(s[2]);
    f.part2.push_back(s[3]);
}
inline G1Affine next_point(size_t idx, const FormattedEntries &f) {   // :1687-1693
    G1Affine p{};
    p.x = recover_basefield(f.part1.at(idx), f.part2.at(idx));
    p.y = recover_basefield(f.part1.at(idx + 1), f.part2.at(idx + 1));
    return p;
}
inline std::string entries_json(const char *k1, const char *k2, const FormattedEntries &f) {
    auto arr = [](const std::vector<std::string> &v) {
        std::string s = "[";
        for (size_t i = 0; i < v.size(); i++) s += (i ? ", \"" : "\"") + v[i] + "\"";
        return s + "]";
    };
    return std::string("{\n  \"") + k1 + "\": " + arr(f.part1) + ",\n  \"" + k2 + "\": " + arr(f.part2) + "\n}\n";
}

}  // namespace tkmk
