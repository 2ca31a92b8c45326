// Host-only dump of what the mask and contour family WOULD launch: every hipLaunchKernelGGL in csrc/contour_hausdorff.hip,
// mask_score.hip, affordance_extract.hip, contour_fill.hip, frame_crop.hip, robot_post.hip and mask_smooth.hip becomes a record in
// text (kernel, grid, block, dynamic LDS bytes, every argument), every hipFuncSetAttribute an `attr` line, every hipMemsetAsync a
// `memset` line and every entry-point call an `rc` line (the workspace functions with their byte count), over a sweep of the eleven
// entry points. The host descriptor tables are real; the device addresses are fake, one 2^40 range per role, never dereferenced, and
// printed as role+offset (a pointer into the workspace is `ws+offset`). Nothing is launched and no GPU is needed.
// The files' anonymous namespaces clash in one unit, so build it once per file (-DDUMP_TU=1..7) and concatenate the outputs; two
// builds against two versions of the sources must print identical output when the host dispatch is unchanged:
//   for t in 1 2 3 4 5 6 7; do hipcc -std=c++17 -x hip --cuda-host-only -Wl,--unresolved-symbols=ignore-all -DDUMP_TU=$t \
//       -I<csrc dir to dump> -Iinclude tools/data_dispatch_dump.cpp -o dump$t; done
//   (for t in 1 2 3 4 5 6 7; do ./dump$t; done) | sha256sum
// A kernel is named by the text at its launch; the kernel of an `attr` line by its address, so a helper may pass it on. Taking a
// kernel's address makes the host-only unit refer to a device binary that is never built: hence the linker flag.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstring>
#include <cctype>
#include <map>
#include <string>
#include <type_traits>
#include <vector>
#undef hipLaunchKernelGGL
#define DUMP_STR(...) #__VA_ARGS__
#define hipLaunchKernelGGL(kernel, grid, block, shmem, stream, ...) dump_launch(DUMP_STR(kernel), grid, block, (size_t)(shmem), __VA_ARGS__)
#define hipGetLastError() hipSuccess
#define hipFuncSetAttribute(fn, attr, value) dump_attr(fn, #attr, (long)(value))
#define hipMemsetAsync(ptr, value, bytes, stream) dump_memset(ptr, value, (size_t)(bytes))
template <typename... A> static void dump_launch(const char* kernel, dim3 g, dim3 b, size_t lds, const A&... a);
static hipError_t dump_attr(const void* fn, const char* attr, long value);
static hipError_t dump_memset(const void* p, int value, size_t bytes);

#ifndef DUMP_TU
#error "build with -DDUMP_TU=1 (contour_hausdorff.hip), 2 (mask_score.hip), 3 (affordance_extract.hip), 4 (contour_fill.hip), 5 (frame_crop.hip), 6 (robot_post.hip) or 7 (mask_smooth.hip)"
#elif DUMP_TU == 1
#include "contour_hausdorff.hip"
#elif DUMP_TU == 2
#include "mask_score.hip"
#elif DUMP_TU == 3
#include "affordance_extract.hip"
#elif DUMP_TU == 4
#include "contour_fill.hip"
#elif DUMP_TU == 5
#include "frame_crop.hip"
#elif DUMP_TU == 6
#include "robot_post.hip"
#else
#include "mask_smooth.hip"
#endif

static long n_records = 0;
static std::map<const void*, const char*> kernel_names;   // for `attr` lines

// fake device addresses: role r (1..15) owns [r << 40, (r + 1) << 40)
static const char* const kRoles[] = {"null", "ws", "planes", "pairs", "verts", "result", "offsets", "summary", "in", "out", "table",
                                     "stats", "hand", "col", "row", "aux"};
enum { WS = 1, PLANES, PAIRS, VERTS, RESULT, OFFSETS, SUMMARY, IN, OUT, TABLE, STATS, HAND, COL, ROW, AUX };
static char* at(unsigned long role, long off = 0) { return reinterpret_cast<char*>(role << 40) + off; }

static void dump_ptr(const void* p) {
  const unsigned long a = reinterpret_cast<unsigned long>(p);
  if (!a) printf(" null");
  else if ((a >> 40) < 16) printf(" %s+%lu", kRoles[a >> 40], a & ((1UL << 40) - 1));
  else printf(" HOST");   // a host address in a kernel argument would be a bug: make it show
}
#if DUMP_TU == 2
static void dump_arg(const ScoreTh& t) {
  for (float v : t.v) printf(" %a", (double)v);
}
#elif DUMP_TU == 6
static void dump_arg(const RobotMaskArgs& p) {
  dump_ptr(p.logits); dump_ptr(p.mask); dump_ptr(p.out);
  printf(" %d %d %d %d %d %d %a %u", p.H0, p.W0, p.Ho, p.Wo, p.left, p.top, (double)p.th, p.on);
}
#endif
template <typename T> static void dump_arg(const T& v) {
  if constexpr (std::is_pointer<T>::value) dump_ptr(v);
  else if constexpr (std::is_floating_point<T>::value) printf(" %a", (double)v);
  else printf(" %lld", (long long)v);
}

template <typename... A> static void dump_launch(const char* kernel, dim3 g, dim3 b, size_t lds, const A&... a) {
  ++n_records;
  std::string k;
  for (const char* c = kernel; *c; ++c)
    if (!isspace((unsigned char)*c) && *c != '(' && *c != ')') k += *c;
  printf("launch %s grid %u %u %u block %u %u %u lds %zu args", k.c_str(), g.x, g.y, g.z, b.x, b.y, b.z, lds);
  (dump_arg(a), ...);
  printf("\n");
}
static hipError_t dump_attr(const void* fn, const char* attr, long value) {
  ++n_records;
  auto it = kernel_names.find(fn);
  printf("attr %s %s %ld\n", it == kernel_names.end() ? "?" : it->second, attr, value);
  return hipSuccess;
}
static hipError_t dump_memset(const void* p, int value, size_t bytes) {
  ++n_records;
  printf("memset");
  dump_ptr(p);
  printf(" %d %zu\n", value, bytes);
  return hipSuccess;
}

// the plane sets of the sweep, (H, W): a pixel, a row, a tile, two odd shapes in one batch, the last plane walked in LDS, the first
// walked in HBM, the largest
static const std::vector<std::vector<std::pair<int, int>>> kSets = {{{1, 1}}, {{1, 64}}, {{32, 32}}, {{33, 65}, {7, 3}}, {{1024, 1024}},
                                                                    {{1025, 1024}}, {{4096, 4096}}};
static std::string set_name(const std::vector<std::pair<int, int>>& set) {
  std::string s;
  for (const auto& hw : set) s += (s.empty() ? "" : "+") + std::to_string(hw.first) + "x" + std::to_string(hw.second);
  return s;
}

#if DUMP_TU == 1
static void sweep() {
  kernel_names[reinterpret_cast<const void*>(contour_walk_kernel)] = "contour_walk_kernel";
  kernel_names[reinterpret_cast<const void*>(extract_walk_kernel<false>)] = "extract_walk_kernel<false>";
  kernel_names[reinterpret_cast<const void*>(extract_walk_kernel<true>)] = "extract_walk_kernel<true>";
  for (const auto& set : kSets) {
    const int n = (int)set.size();
    std::vector<Plane> pl(n);
    long pixels = 0;
    for (int i = 0; i < n; ++i) {
      pl[i] = Plane{reinterpret_cast<const unsigned char*>(at(PLANES, 1L << 30)) + pixels, set[i].first, set[i].second};
      pixels += (long)set[i].first * set[i].second;
    }
    std::vector<int> pairs;
    for (int i = 0; i < n; ++i) { pairs.push_back(i); pairs.push_back(i); }
    pairs.push_back(n - 1); pairs.push_back(0);          // of unequal shapes in the mixed batch: dropped below unless n == 1
    const std::string name = set_name(set);
    for (int mv : {1, 65536}) {
      long need = -1;
      int rc = haff_contour_hausdorff_workspace(pl.data(), n, mv, &need);
      printf("rc hausdorff_workspace %s mv %d -> %d bytes %ld\n", name.c_str(), mv, rc, need);
      for (int vo = 0; vo < 2; ++vo)
        for (int np : {n, n + 1}) {
          if (np > n && n > 1) continue;
          rc = haff_contour_hausdorff(pl.data(), at(PLANES), n, pairs.data(), reinterpret_cast<const int*>(at(PAIRS)), np, mv, at(WS), need,
                                      vo ? at(VERTS) : nullptr, at(RESULT), nullptr);
          printf("rc hausdorff %s mv %d pairs %d verts_out %d -> %d\n", name.c_str(), mv, np, vo, rc);
        }
      printf("rc hausdorff %s mv %d short -> %d\n", name.c_str(), mv,
             haff_contour_hausdorff(pl.data(), at(PLANES), n, pairs.data(), reinterpret_cast<const int*>(at(PAIRS)), n, mv, at(WS), need - 1,
                                    nullptr, at(RESULT), nullptr));
      for (int mc : {1, 4, 5, 1024}) {
        need = -1;
        rc = haff_contour_extract_workspace(pl.data(), n, mc, mv, &need);
        printf("rc extract_workspace %s mc %d mv %d -> %d bytes %ld\n", name.c_str(), mc, mv, rc, need);
        rc = haff_contour_extract(pl.data(), at(PLANES), n, mc, mv, at(WS), need, at(VERTS), at(OFFSETS), at(SUMMARY), nullptr);
        printf("rc extract %s mc %d mv %d -> %d\n", name.c_str(), mc, mv, rc);
        printf("rc extract %s mc %d mv %d short -> %d\n", name.c_str(), mc, mv,
               haff_contour_extract(pl.data(), at(PLANES), n, mc, mv, at(WS), need - 1, at(VERTS), at(OFFSETS), at(SUMMARY), nullptr));
      }
    }
  }
}

#elif DUMP_TU == 2
static void sweep() {
  float ths[8] = {-2.f, -1.f, -.5f, 0.f, .25f, .5f, 1.f, 2.f};
  for (const auto& set : kSets) {
    const int n = (int)set.size();
    for (int form = 0; form < 3; ++form) {                // logits of the planes' size; of another; one hand, no taxonomy, no planes out
      std::vector<ScoreFrame> fr(n);
      for (int i = 0; i < n; ++i) {
        ScoreFrame f{};
        f.Hb = set[i].first; f.Wb = set[i].second;
        f.Hs = form == 1 ? 256 : f.Hb; f.Ws = form == 1 ? 192 : f.Wb;
        f.logit[0] = reinterpret_cast<const float*>(at(IN, 64L * i));
        f.logit[1] = form == 2 ? nullptr : reinterpret_cast<const float*>(at(IN, (1L << 30) + 64L * i));
        if (form != 2) { f.tax = reinterpret_cast<const float*>(at(AUX, 16L * i)); f.n_tax = 4; }
        for (int h = 0; h < 2; ++h) {
          f.gt[h] = reinterpret_cast<const unsigned char*>(at(PLANES, (long)h << 30));
          f.gt_hw[h][0] = f.Hb; f.gt_hw[h][1] = f.Wb;
          if (form == 0) { f.obj[h] = reinterpret_cast<const unsigned char*>(at(HAND, (long)h << 30)); f.obj_hw[h][0] = f.Hb; f.obj_hw[h][1] = f.Wb; }
        }
        f.out = form == 2 ? nullptr : reinterpret_cast<unsigned char*>(at(OUT));
        fr[i] = f;
      }
      for (int n_th : {1, 3, 8})
        printf("rc score_masks %s form %d n_th %d -> %d\n", set_name(set).c_str(), form, n_th,
               haff_score_masks(fr.data(), at(TABLE), n, ths, n_th, at(RESULT), nullptr));
    }
  }
}

#elif DUMP_TU == 3
static void sweep() {
  for (const auto& set : kSets) {
    const int n = (int)set.size();
    for (int form = 0; form < 3; ++form) {                // plane and out; with a hand; statistics only
      std::vector<ExtractItem> items(n);
      for (int i = 0; i < n; ++i) {
        ExtractItem it{};
        it.in = reinterpret_cast<const unsigned char*>(at(IN, (long)i << 30));
        it.out = form == 2 ? nullptr : reinterpret_cast<unsigned char*>(at(OUT, (long)i << 30));
        it.H = set[i].first; it.W = set[i].second;
        if (form == 1) {
          it.hand = reinterpret_cast<const unsigned char*>(at(HAND));
          it.col = reinterpret_cast<const int*>(at(COL));
          it.row = reinterpret_cast<const int*>(at(ROW));
          it.Hh = 48; it.Wh = 4096;
        }
        items[i] = it;
      }
      for (int k : {1, 2, 31})
        printf("rc affordance_extract %s form %d k %d -> %d\n", set_name(set).c_str(), form, k,
               haff_affordance_extract(items.data(), at(TABLE), n, k, at(STATS), nullptr));
    }
  }
}

#elif DUMP_TU == 4
static void sweep() {
  // polygons: none; one point; a triangle and a point on two planes; a 4096-gon
  struct Case { const char* name; std::vector<int> off, plane, pts; int n_planes; };
  std::vector<Case> cases = {{"none", {0}, {}, {}, 1}, {"point", {0, 1}, {0}, {0, 0}, 1},
                             {"triangle+point", {0, 3, 4}, {1, 0}, {0, 0, 5, 0, 0, 5, 2, 2}, 2}, {"4096-gon", {0, 4096}, {2}, {}, 3}};
  for (int i = 0; i < 4096; ++i) { cases[3].pts.push_back(i % 64); cases[3].pts.push_back(i / 64); }
  for (const auto& set : kSets)
    for (const auto& hw : set)
      for (const auto& c : cases)
        printf("rc fill_contours %dx%d %s -> %d\n", hw.first, hw.second, c.name,
               haff_fill_contours_u8(c.pts.data(), c.off.data(), c.plane.data(), reinterpret_cast<const int*>(at(TABLE)), (int)c.plane.size(),
                                     c.n_planes, at(OUT), hw.first, hw.second, nullptr));
}

#elif DUMP_TU == 5
static void sweep() {
  for (const auto& set : kSets)
    for (const auto& hw : set)
      for (int C : {1, 3})
        for (int form = 0; form < 3; ++form) {              // copies; mirrors; sample 0 cropped to its whole self (one tap per row)
          const int H = hw.first, W = hw.second, B = 3, S = H > W ? H : W;
          if (form == 2 && (long)H * W > 1 << 20) continue;
          std::vector<int> d(B * HAFF_CROP_GEOM, 0);
          if (form == 1) d[7] = d[HAFF_CROP_GEOM + 7] = 1;
          if (form == 2) {
            const int g[12] = {0, 0, W, H, 0, 0, S, 4, (int)d.size(), 1, (int)d.size() + 3 * W, 1};
            memcpy(d.data(), g, sizeof g);
            for (int i = 0; i < W; ++i) { d.push_back(i); d.push_back(1); d.push_back(1 << 22); }
            for (int i = 0; i < H; ++i) { d.push_back(i); d.push_back(1); d.push_back(1 << 22); }
          }
          printf("rc crop_resample %dx%d C %d form %d -> %d\n", H, W, C, form,
                 haff_crop_resample_u8(at(IN), at(OUT), B, H, W, C, d.data(), reinterpret_cast<const int*>(at(TABLE)), (long)d.size(), nullptr));
        }
}

#elif DUMP_TU == 6
static void sweep() {
  for (const auto& set : kSets)
    for (const auto& hw : set) {
      const int H = hw.first, W = hw.second;
      for (int n : {1, 3})
        for (int mis : {0, 4, 2})                           // logits on a 16-byte boundary, on a 4-byte one, on neither
          printf("rc robot_heatmap %dx%d n %d logits+%d -> %d\n", H, W, n, mis,
                 haff_robot_heatmap(reinterpret_cast<const float*>(at(IN, mis)), n, H, W, at(TABLE), reinterpret_cast<float*>(at(WS)),
                                    (long)n * 512, at(OUT), nullptr));
      printf("rc robot_heatmap %dx%d workspace short -> %d\n", H, W,
             haff_robot_heatmap(reinterpret_cast<const float*>(at(IN)), 2, H, W, at(TABLE), reinterpret_cast<float*>(at(WS)), 1023, at(OUT),
                                nullptr));
      const int margins[][4] = {{0, 0, 0, 0}, {3, 5, 7, 11}, {-1, 0, 0, -1}, {0, -H, 0, 0}};
      for (const auto& m : margins)
        for (int mask = 0; mask < 3; ++mask) {              // none; of the padded size; one row short
          const long Ho = (long)H + m[1] + m[3], Wo = (long)W + m[0] + m[2];
          printf("rc robot_mask %dx%d margins %d %d %d %d mask %d -> %d\n", H, W, m[0], m[1], m[2], m[3], mask,
                 haff_robot_mask(reinterpret_cast<const float*>(at(IN)), H, W, m[0], m[1], m[2], m[3], 0.25f, mask ? at(HAND) : nullptr,
                                 (int)Ho - (mask == 2), (int)Wo, 255, at(OUT), nullptr));
        }
    }
}

#else
static void sweep() {
  for (const auto& set : kSets)
    for (const auto& hw : set)
      for (int n : {1, 3, 70000})
        for (int mis : {0, 4, 2})
          for (int need : {1, 32768, 65536, 65537})
            printf("rc mask_quantile7 %dx%d n %d logits+%d need %d -> %d\n", hw.first, hw.second, n, mis, need,
                   haff_mask_quantile7(reinterpret_cast<const float*>(at(IN, mis)), n, hw.first, hw.second, need,
                                       reinterpret_cast<float*>(at(OUT)), nullptr));
}
#endif

int main() {
  sweep();
  fprintf(stderr, "%ld records\n", n_records);
  return 0;
}
