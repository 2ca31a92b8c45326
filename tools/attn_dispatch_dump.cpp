// Host-only dump of what the attention family WOULD launch: every hipLaunchKernelGGL in csrc/attention.hip, attention_f32.hip,
// attention_bwd.hip and window_attention.hip becomes a record in text (the kernel instance with every template argument as a value,
// grid, block, dynamic LDS bytes, every field of the argument struct by name or each loose argument), every hipFuncSetAttribute an
// `attr` line and every entry-point call an `rc` line, over a sweep of all 18 entry points. Nothing is launched and no GPU is needed.
// The four files' anonymous namespaces clash in one unit, so build it once per file (-DDUMP_TU=1..4) and concatenate the outputs; two
// builds against two versions of the sources must print identical output when the host dispatch is unchanged:
//   for t in 1 2 3 4; do hipcc -std=c++17 -x hip --cuda-host-only -DDUMP_TU=$t -I<csrc dir to dump> -Iinclude tools/attn_dispatch_dump.cpp -o dump$t; done
//   (./dump1; ./dump2; ./dump3; ./dump4) | sha256sum
// A record does not depend on which host function launches: the kernel expression as written at the launch has the launching
// function's template arguments (from __PRETTY_FUNCTION__) substituted into it.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstring>
#include <cctype>
#include <map>
#include <set>
#include <string>
#undef hipLaunchKernelGGL
#define DUMP_STR(...) #__VA_ARGS__
#define hipLaunchKernelGGL(kernel, grid, block, shmem, stream, ...) \
  dump_launch(DUMP_STR(kernel), __PRETTY_FUNCTION__, grid, block, (size_t)(shmem), __VA_ARGS__)
#define hipGetLastError() hipSuccess
#define hipFuncSetAttribute(fn, attr, value) dump_attr(DUMP_STR(fn), __PRETTY_FUNCTION__, #attr, (long)(value))
template <typename... A> static void dump_launch(const char* kernel, const char* pretty, dim3 g, dim3 b, size_t lds, const A&... a);
static hipError_t dump_attr(const char* fn, const char* pretty, const char* attr, long value);

#ifndef DUMP_TU
#error "build with -DDUMP_TU=1 (attention.hip), 2 (attention_f32.hip), 3 (attention_bwd.hip) or 4 (window_attention.hip)"
#elif DUMP_TU == 1
#include "attention.hip"
#elif DUMP_TU == 2
#include "attention_f32.hip"
#elif DUMP_TU == 3
#include "attention_bwd.hip"
#else
#include "window_attention.hip"
#endif

static long n_records = 0;
static std::set<std::string> instances;

// "(attn_fwd_kernel<DP, BIAS, F16>)" written in "... [DP = 64, BIAS = 3, F16 = false]" -> "attn_fwd_kernel<64,3,false>"
static std::string resolve(const char* text, const char* pretty) {
  std::map<std::string, std::string> sub;
  if (const char* lb = strrchr(pretty, '[')) {
    std::string s(lb + 1);
    if (!s.empty() && s.back() == ']') s.pop_back();
    size_t pos = 0;
    while (pos < s.size()) {
      size_t end = s.find(", ", pos);
      if (end == std::string::npos) end = s.size();
      const std::string item = s.substr(pos, end - pos);
      const size_t eq = item.find(" = ");
      if (eq != std::string::npos) sub[item.substr(0, eq)] = item.substr(eq + 3);
      pos = end + 2;
    }
  }
  std::string t;
  for (const char* c = text; *c; ++c)
    if (!isspace((unsigned char)*c)) t += *c;
  const std::string cast = "reinterpret_cast<constvoid*>(";
  if (t.compare(0, cast.size(), cast) == 0) t = t.substr(cast.size(), t.size() - cast.size() - 1);
  while (!t.empty() && (t[0] == '(' || t[0] == '&')) {
    if (t[0] == '(') t.pop_back();
    t.erase(0, 1);
  }
  std::string out;
  for (size_t i = 0; i < t.size();) {
    if (isalpha((unsigned char)t[i]) || t[i] == '_') {
      size_t j = i;
      while (j < t.size() && (isalnum((unsigned char)t[j]) || t[j] == '_')) ++j;
      const std::string id = t.substr(i, j - i);
      auto it = sub.find(id);
      out += it == sub.end() ? id : it->second;
      i = j;
    } else {
      out += t[i++];
    }
  }
  return out;
}

static void dump_arg(const void* p) { printf(" %p", p); }
static void dump_arg(long v) { printf(" %ld", v); }
static void dump_arg(int v) { printf(" %d", v); }
static void dump_arg(float v) { printf(" %a", (double)v); }
#if DUMP_TU == 1
static void dump_arg(const AttnArgs& p) {
  printf("\n q %p k %p v %p o %p q_s %ld %ld %ld k_s %ld %ld %ld v_s %ld %ld %ld o_s %ld %ld %ld B %d H %d Nq %d Nk %d d %d scale %a q_pos0 %d",
         (const void*)p.q, (const void*)p.k, (const void*)p.v, (const void*)p.o, p.q_sb, p.q_sh, p.q_st, p.k_sb, p.k_sh, p.k_st, p.v_sb,
         p.v_sh, p.v_st, p.o_sb, p.o_sh, p.o_st, p.B, p.H, p.Nq, p.Nk, p.d, (double)p.scale, p.q_pos0);
  printf("\n relh %p relw %p S %d nk_rows %p knew %p vnew %p cos_sin %p tab_h %p tab_w %p lse %p", (const void*)p.relh, (const void*)p.relw,
         p.S, (const void*)p.nk_rows, (const void*)p.knew, (const void*)p.vnew, (const void*)p.cos_sin, (const void*)p.tab_h,
         (const void*)p.tab_w, (const void*)p.lse);
}
#elif DUMP_TU == 2
static void dump_arg(const AttnF32Args& p) {
  printf("\n q %p k %p v %p o %p q_s %ld %ld %ld k_s %ld %ld %ld v_s %ld %ld %ld o_s %ld %ld %ld B %d H %d Nq %d Nk %d d %d scale %a causal %d"
         " q_pos0 %d relh %p relw %p S %d nk_rows %p", (const void*)p.q, (const void*)p.k, (const void*)p.v, (const void*)p.o, p.q_sb,
         p.q_sh, p.q_st, p.k_sb, p.k_sh, p.k_st, p.v_sb, p.v_sh, p.v_st, p.o_sb, p.o_sh, p.o_st, p.B, p.H, p.Nq, p.Nk, p.d, (double)p.scale,
         p.causal, p.q_pos0, (const void*)p.relh, (const void*)p.relw, p.S, (const void*)p.nk_rows);
}
#elif DUMP_TU == 3
static void dump_arg(const BwdArgs& p) {
  printf("\n q %p k %p v %p dout %p lse %p delta %p dq %p dk %p dv %p dq_acc %p ld %ld B %d H %d Nq %d Nk %d scale %a causal %d q_pos0 %d",
         (const void*)p.q, (const void*)p.k, (const void*)p.v, (const void*)p.dout, (const void*)p.lse, (const void*)p.delta,
         (const void*)p.dq, (const void*)p.dk, (const void*)p.dv, (const void*)p.dq_acc, p.ld, p.B, p.H, p.Nq, p.Nk, (double)p.scale,
         p.causal, p.q_pos0);
}
#else
static void dump_arg(const WinArgs& p) {
  printf("\n q %p k %p v %p o %p q_s %ld %ld %ld k_s %ld %ld %ld v_s %ld %ld %ld o_s %ld %ld %ld B %d H %d scale %a tab_h %p tab_w %p"
         " grid %d %d wps %d pad_token %ld", (const void*)p.q, (const void*)p.k, (const void*)p.v, (const void*)p.o, p.q_sb, p.q_sh,
         p.q_st, p.k_sb, p.k_sh, p.k_st, p.v_sb, p.v_sh, p.v_st, p.o_sb, p.o_sh, p.o_st, p.B, p.H, (double)p.scale, (const void*)p.tab_h,
         (const void*)p.tab_w, p.grid_h, p.grid_w, p.wps, p.pad_token);
}
#endif

template <typename... A> static void dump_launch(const char* kernel, const char* pretty, dim3 g, dim3 b, size_t lds, const A&... a) {
  ++n_records;
  const std::string k = resolve(kernel, pretty);
  instances.insert(k);
  printf("launch %s grid %u %u %u block %u %u %u lds %zu args", k.c_str(), g.x, g.y, g.z, b.x, b.y, b.z, lds);
  (dump_arg(a), ...);
  printf("\n");
}
static hipError_t dump_attr(const char* fn, const char* pretty, const char* attr, long value) {
  printf("attr %s %s %ld\n", resolve(fn, pretty).c_str(), attr, value);
  return hipSuccess;
}

// fake device addresses (never dereferenced), one per role; `off` in bytes
static char* at(unsigned long a, long off = 0) { return reinterpret_cast<char*>(a << 32) + off; }

struct Lay {   // (batch, head, token) strides in elements and the four operand bases
  const char* name;
  char *q, *k, *v, *o;
  long q_sb, q_sh, q_st, k_sb, k_sh, k_st, v_sb, v_sh, v_st, o_sb, o_sh, o_st;
};
// kind 0: q|k|v rows of one fused projection (token-major, as sam.py and llava.py pass them); 1: separate head-major planes;
// 2: fused with v BEFORE k; 3: planes with another token stride for v; 4: fused with a 2^19-element token stride.
// okind 0: token-major output; 1: head stride d + 4 (8-byte rows only); 2: base 8 bytes off a 16-byte boundary
static Lay layout(int kind, int okind, int esz, int H, long Nq, long Nk, int d) {
  Lay l{};
  static const char* names[] = {"fused", "planes", "fused-vk", "planes-vst", "fused-wide"};
  l.name = names[kind];
  const long hd = (long)H * d;
  if (kind == 1 || kind == 3) {
    l.q = at(1); l.k = at(2); l.v = at(3);
    l.q_sb = H * Nq * d; l.q_sh = Nq * d; l.q_st = d;
    l.k_sb = l.v_sb = H * Nk * d; l.k_sh = l.v_sh = Nk * d; l.k_st = l.v_st = d;
    if (kind == 3) l.v_st = 2 * d;
  } else {
    const long row = kind == 4 ? (1L << 19) : 3 * hd;
    l.q = at(1); l.k = at(1, hd * esz); l.v = at(1, 2 * hd * esz);
    if (kind == 2) { l.k = at(1, 2 * hd * esz); l.v = at(1, hd * esz); }
    l.q_sb = Nq * row; l.k_sb = l.v_sb = Nk * row;
    l.q_sh = l.k_sh = l.v_sh = d;
    l.q_st = l.k_st = l.v_st = row;
  }
  l.o = at(4, okind == 2 ? 8 : 0);
  l.o_sh = okind == 1 ? d + 4 : d;
  l.o_st = (long)H * l.o_sh;
  l.o_sb = Nq * l.o_st;
  return l;
}
#define LAY16(l) (l).q, (l).q_sb, (l).q_sh, (l).q_st, (l).k, (l).k_sb, (l).k_sh, (l).k_st, (l).v, (l).v_sb, (l).v_sh, (l).v_st, (l).o, (l).o_sb, (l).o_sh, (l).o_st
static const int BH[][2] = {{1, 2}, {8, 16}, {3, 43}, {32, 32}, {25, 41}};   // B*H = 2, 128, 129, 1024, 1025

#if DUMP_TU == 1
static float* REL(int which, int off) { return reinterpret_cast<float*>(at(5 + which, off)); }
static int* NKR = reinterpret_cast<int*>(at(7));
static float* LSE = reinterpret_cast<float*>(at(8));

template <bool F16> static void sweep_attention() {
  auto fn = F16 ? haff_attention_f16 : haff_attention_bf16;
  auto fn_lse = F16 ? haff_attention_lse_f16 : haff_attention_lse_bf16;
  const int ds[] = {8, 16, 32, 64, 72, 80, 96, 104, 128};
  const int shapes[][2] = {{1, 1}, {1, 300}, {100, 100}, {128, 64}, {128, 128}, {196, 196}, {256, 192}, {257, 257}, {291, 291}, {196, 392},
                           {300, 4096}, {4096, 4096}, {1024, 1024}, {49, 49}};
  for (int d : ds)
    for (const auto& sh : shapes)
      for (int bh = 0; bh < (sh[0] == 1 ? 5 : 2); ++bh)
        for (int kind = 0; kind < (sh[1] == 4096 ? 5 : 2); ++kind)
          for (int okind = 0; okind < 3; ++okind) {
            const int B = BH[bh][0], H = BH[bh][1], Nq = sh[0], Nk = sh[1];
            const Lay l = layout(kind, okind, 2, H, Nq, Nk, d);
            const float scale = 1.f / (float)d;
            const int qp[][2] = {{0, 0}, {1, 0}, {1, Nk - 2}, {1, Nk - 1}, {1, Nk}};
            for (const auto& c : qp) {
              printf("rc attention f16=%d %s o%d B %d H %d Nq %d Nk %d d %d causal %d q_pos0 %d -> %d\n", (int)F16, l.name, okind, B, H, Nq,
                     Nk, d, c[0], c[1], fn(LAY16(l), B, H, Nq, Nk, d, scale, c[0], c[1], nullptr, nullptr, 0, nullptr));
              if (kind == 0 && bh == 0)
                printf("rc attention_lse f16=%d %s o%d B %d H %d Nq %d Nk %d d %d causal %d q_pos0 %d -> %d\n", (int)F16, l.name, okind, B, H,
                       Nq, Nk, d, c[0], c[1], fn_lse(LAY16(l), B, H, Nq, Nk, d, scale, c[0], c[1], LSE, nullptr));
            }
            if (bh > 1) continue;
            for (int S : {7, 14, 16, 28, 32, 40, 64})
              for (int mis = 0; mis < 3; ++mis) {   // rel-pos tables aligned, relh 4 bytes off, relw 4 bytes off
                if (Nk % S) continue;
                printf("rc attention f16=%d %s o%d B %d H %d Nq %d Nk %d d %d rel S %d mis %d -> %d\n", (int)F16, l.name, okind, B, H, Nq, Nk,
                       d, S, mis, fn(LAY16(l), B, H, Nq, Nk, d, scale, 0, 0, REL(0, mis == 1 ? 4 : 0), REL(1, mis == 2 ? 4 : 0), S, nullptr));
              }
            // one table only: no rel-pos
            printf("rc attention f16=%d %s o%d B %d H %d Nq %d Nk %d d %d relh only -> %d\n", (int)F16, l.name, okind, B, H, Nq, Nk, d,
                   fn(LAY16(l), B, H, Nq, Nk, d, scale, 0, 0, REL(0, 0), nullptr, 14, nullptr));
          }
}

template <bool F16> static void sweep_global() {
  auto fn = F16 ? haff_global_attention_f16 : haff_global_attention_bf16;
  for (int S : {14, 32, 64})
    for (int d : {64, 80})
      for (int bh = 0; bh < 2; ++bh)
        for (int kind = 0; kind < 5; ++kind)
          for (int okind = 0; okind < 3; ++okind)
            for (int tab = 0; tab < 4; ++tab) {   // tables aligned, tab_h 8 bytes off, tab_w 8 bytes off, tab_w null
              const int B = BH[bh][0], H = BH[bh][1];
              const Lay l = layout(kind, okind, 2, H, S * S, S * S, d);
              printf("rc global f16=%d %s o%d B %d H %d S %d d %d tab %d -> %d\n", (int)F16, l.name, okind, B, H, S, d, tab,
                     fn(LAY16(l), B, H, S, d, 0.125f, at(9, tab == 1 ? 8 : 0), tab == 3 ? nullptr : at(10, tab == 2 ? 8 : 0), nullptr));
            }
}

template <bool F16> static void sweep_decode() {
  auto rows = F16 ? haff_attention_decode_rows_f16 : haff_attention_decode_rows_bf16;
  auto rope = F16 ? haff_decode_attention_rope_rows_f16 : haff_decode_attention_rope_rows_bf16;
  for (int d : {64, 128})
    for (int Nk : {1, 300, 4096})
      for (const auto& bh : BH)
        for (int kind = 0; kind < 2; ++kind)
          for (int okind = 0; okind < 3; ++okind)
            for (int nkr = 0; nkr < 2; ++nkr) {
              const int B = bh[0], H = bh[1];
              const Lay l = layout(kind, okind, 2, H, 1, Nk, d);
              printf("rc decode_rows f16=%d %s o%d B %d H %d Nk %d d %d nk_rows %d -> %d\n", (int)F16, l.name, okind, B, H, Nk, d, nkr,
                     rows(l.q, l.q_sb, l.q_sh, l.k, l.k_sb, l.k_sh, l.k_st, l.v, l.v_sb, l.v_sh, l.v_st, l.o, l.o_sb, l.o_sh, B, H, Nk, d,
                          0.25f, nkr ? NKR : nullptr, nullptr));
            }
  for (int d : {64, 128})
    for (int Tmax : {1, 1024})
      for (const auto& bh : BH)
        for (int ldx : {0, 8, 4})
          for (int mis = 0; mis < 7; ++mis) {   // 1..4: qkv / kcache / vcache / out 8 bytes off; 5: no nk_rows; 6: no cos_sin
            const int B = bh[0], H = bh[1];
            printf("rc rope_rows f16=%d B %d H %d d %d Tmax %d ld+%d mis %d -> %d\n", (int)F16, B, H, d, Tmax, ldx, mis,
                   rope(at(1, mis == 1 ? 8 : 0), 3L * H * d + ldx, at(2, mis == 2 ? 8 : 0), at(3, mis == 3 ? 8 : 0),
                        mis == 6 ? nullptr : REL(0, 0), at(4, mis == 4 ? 8 : 0), B, H, d, Tmax, 0.25f, mis == 5 ? nullptr : NKR, nullptr));
          }
}

static void sweep_relpos() {
  for (int S : {7, 14, 32, 64, 120, 121, 296, 297})   // 121: the first above the 64 KB attribute line; 297: the first refused
    for (int d : {8, 32, 40, 64, 80, 96, 104, 128, 136})
      for (int bh = 0; bh < 2; ++bh)
        for (long q_st : {(long)d, 3L * BH[bh][1] * d, (long)d + 4}) {
          const int B = BH[bh][0], H = BH[bh][1];
          printf("rc relpos_tables_bf16 B %d H %d S %d d %d q_st %ld -> %d\n", B, H, S, d, q_st,
                 haff_relpos_tables_bf16(at(1), (long)S * S * H * q_st, d, q_st, at(9), at(10), REL(0, 0), REL(1, 0), B, H, S, d, nullptr));
          for (int dtype : {0, 1, 2, 3})
            printf("rc relpos_tables B %d H %d S %d d %d q_st %ld dtype %d -> %d\n", B, H, S, d, q_st, dtype,
                   haff_relpos_tables(at(1), (long)S * S * H * q_st, d, q_st, REL(2, 0), REL(3, 0), REL(0, 0), REL(1, 0), B, H, S, d, dtype,
                                      nullptr));
        }
}

static void sweep() {
  sweep_attention<false>();
  sweep_attention<true>();
  sweep_global<false>();
  sweep_global<true>();
  sweep_decode<false>();
  sweep_decode<true>();
  sweep_relpos();
}

#elif DUMP_TU == 2
static void sweep() {
  float* relh = reinterpret_cast<float*>(at(5));
  float* relw = reinterpret_cast<float*>(at(6));
  int* nkr = reinterpret_cast<int*>(at(7));
  // few-keys form: no bias, no mask, Nk <= 16, Nq >= 256, d 16 / 32 (the mask decoder's image-to-token attentions)
  const int shapes[][2] = {{1, 1}, {7, 4096}, {4096, 7}, {256, 16}, {255, 16}, {256, 17}, {257, 257}, {196, 196}, {4096, 4096}, {5, 9280},
                           {5, 9281}, {5, 9312}, {5, 9313}, {2, 20000}};
  for (int d : {4, 16, 32, 64, 80, 256, 260})
    for (const auto& sh : shapes)
      for (int bh = 0; bh < 2; ++bh)
        for (int kind = 0; kind < 2; ++kind) {
          const int B = BH[bh][0], H = BH[bh][1], Nq = sh[0], Nk = sh[1];
          const Lay l = layout(kind, 0, 4, H, Nq, Nk, d);
#define LAY16F(l) (const float*)(l).q, (l).q_sb, (l).q_sh, (l).q_st, (const float*)(l).k, (l).k_sb, (l).k_sh, (l).k_st, (const float*)(l).v, (l).v_sb, (l).v_sh, (l).v_st, (float*)(l).o, (l).o_sb, (l).o_sh, (l).o_st
          const int qp[][2] = {{0, 0}, {0, 5}, {1, 0}, {1, Nk - 1}};
          for (const auto& c : qp)
            printf("rc attention_f32 %s B %d H %d Nq %d Nk %d d %d causal %d q_pos0 %d -> %d\n", l.name, B, H, Nq, Nk, d, c[0], c[1],
                   haff_attention_f32(LAY16F(l), B, H, Nq, Nk, d, 0.25f, c[0], c[1], nullptr, nullptr, 0, nullptr));
          for (int S : {0, 1, 14, 16, 64}) {
            printf("rc attention_f32 %s B %d H %d Nq %d Nk %d d %d rel S %d -> %d\n", l.name, B, H, Nq, Nk, d, S,
                   haff_attention_f32(LAY16F(l), B, H, Nq, Nk, d, 0.25f, 0, 0, relh, relw, S, nullptr));
            printf("rc attention_f32 %s B %d H %d Nq %d Nk %d d %d causal rel S %d -> %d\n", l.name, B, H, Nq, Nk, d, S,
                   haff_attention_f32(LAY16F(l), B, H, Nq, Nk, d, 0.25f, 1, 3, relh, relw, S, nullptr));
            printf("rc attention_f32 %s B %d H %d Nq %d Nk %d d %d relw only S %d -> %d\n", l.name, B, H, Nq, Nk, d, S,
                   haff_attention_f32(LAY16F(l), B, H, Nq, Nk, d, 0.25f, 0, 2, nullptr, relw, S, nullptr));
          }
          if (Nq == sh[0] && bh == 0)
            for (int nk = 0; nk < 2; ++nk)
              printf("rc decode_rows_f32 %s B %d H %d Nk %d d %d nk_rows %d -> %d\n", l.name, B, H, Nk, d, nk,
                     haff_attention_decode_rows_f32((const float*)l.q, l.q_sb, l.q_sh, (const float*)l.k, l.k_sb, l.k_sh, l.k_st,
                                                    (const float*)l.v, l.v_sb, l.v_sh, l.v_st, (float*)l.o, l.o_sb, l.o_sh, B, H, Nk, d, 0.25f,
                                                    nk ? nkr : nullptr, nullptr));
        }
  // the stride rule of the f32 family: multiples of 4 elements
  const Lay l = layout(1, 0, 4, 2, 64, 64, 32);
  for (int which = 0; which < 12; ++which) {
    Lay m = l;
    (&m.q_sb)[which] += 2;
    printf("rc attention_f32 stride %d off -> %d\n", which, haff_attention_f32(LAY16F(m), 1, 2, 64, 64, 32, 0.25f, 0, 0, nullptr, nullptr, 0, nullptr));
  }
}

#elif DUMP_TU == 3
template <bool F16> static void sweep_bwd() {
  auto fn = F16 ? haff_attention_bwd_f16 : haff_attention_bwd_bf16;
  const int shapes[][2] = {{1, 1}, {63, 65}, {64, 64}, {100, 291}, {291, 291}, {2808, 2808}, {128, 1}};
  float* lse = reinterpret_cast<float*>(at(6));
  for (const auto& bh : {BH[0], BH[1], BH[2]})
    for (const auto& sh : shapes)
      for (int d : {64, 128})
        for (int ldx : {0, 128, 4, -128})
          for (int ws = 0; ws < 4; ++ws)     // workspace exact, one short, 8 bytes off, null
            for (int mis = 0; mis < 3; ++mis) {   // 1: dq 8 bytes off; 2: lse null
              const int B = bh[0], H = bh[1], Nq = sh[0], Nk = sh[1];
              const long nqp = (long)((Nq + 63) / 64) * 64;
              const long need = (((long)B * H * Nq + 3) / 4) * 4 + (long)B * H * nqp * 128;
              const int qp[][2] = {{0, 0}, {1, 0}, {1, 7}, {1, -1}};
              for (const auto& c : qp)
                printf("rc attention_bwd f16=%d B %d H %d Nq %d Nk %d d %d ld+%d ws %d mis %d causal %d q_pos0 %d -> %d\n", (int)F16, B, H, Nq,
                       Nk, d, ldx, ws, mis, c[0], c[1],
                       fn(at(1), at(2), at(3), at(4), at(5), mis == 2 ? nullptr : lse, at(7, mis == 1 ? 8 : 0), at(8), at(9),
                          ws == 3 ? nullptr : reinterpret_cast<float*>(at(10, ws == 2 ? 8 : 0)), ws == 1 ? need - 1 : need, (long)H * 128 + ldx,
                          B, H, Nq, Nk, d, 0.088f, c[0], c[1], nullptr));
            }
}
static void sweep() {
  sweep_bwd<false>();
  sweep_bwd<true>();
}

#else
template <bool F16> static void sweep_window() {
  auto fn = F16 ? haff_window_attention_f16 : haff_window_attention_bf16;
  // grids: none; 64 tokens (5 x 5 windows of 14, SAM's 1024-pixel frames); 63; one window; not square
  const int grids[][2] = {{0, 0}, {64, 64}, {63, 63}, {14, 14}, {64, 56}};
  for (int S : {7, 14})
    for (int d : {64, 80})
      for (int nw : {1, 25, 50, 800})
        for (int H : {2, 16})
          for (int kind = 0; kind < 5; ++kind)
            for (int okind = 0; okind < 3; ++okind)
              for (const auto& g : grids)
                for (int tab = 0; tab < 4; ++tab) {   // tables aligned, tab_h 8 bytes off, tab_w 8 bytes off, tab_w null
                  const Lay l = layout(kind, okind, 2, H, S * S, S * S, d);
                  // the pad row: behind the last window (as sam.py places it), inside the windows, absent, or past 4 GiB
                  const long pads[] = {(long)nw * S * S, 3, -1, (1L << 32) / (l.k_st * 2)};
                  for (int pi = 0; pi < (g[0] ? 4 : 1); ++pi)
                    printf("rc window f16=%d %s o%d nw %d H %d S %d d %d grid %d %d pad %d tab %d -> %d\n", (int)F16, l.name, okind, nw, H, S,
                           d, g[0], g[1], pi, tab,
                           fn(LAY16(l), nw, H, S, d, 0.1118f, at(9, tab == 1 ? 8 : 0), tab == 3 ? nullptr : at(10, tab == 2 ? 8 : 0), g[0],
                              g[1], pads[pi], nullptr));
                }
  // operand bases off their boundaries, one at a time
  for (int which = 0; which < 4; ++which) {
    Lay l = layout(0, 0, 2, 16, 196, 196, 80);
    (&l.q)[which] += 8;
    printf("rc window f16=%d base %d off -> %d\n", (int)F16, which, fn(LAY16(l), 25, 16, 14, 80, 0.1118f, at(9), at(10), 0, 0, 0, nullptr));
  }
}
static void sweep() {
  sweep_window<false>();
  sweep_window<true>();
}
#endif

int main() {
  sweep();
  fprintf(stderr, "%ld launch records, %zu kernel instances\n", n_records, instances.size());
  for (const auto& k : instances) fprintf(stderr, "  %s\n", k.c_str());
  return 0;
}
