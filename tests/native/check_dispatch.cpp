// kmeans-gpu_amd/csrc/kmg_dispatch.h on its own: no device, nothing of HIP.
//   every helper calls f exactly once, with the tag of its input, for every input it lists, and says so (true);
//   for an input it does not list it calls nothing and says so (false);
//   the nests the launchers use map the full cross product of their runtime inputs onto as many DISTINCT template tuples, each
//   equal to its inputs -- stand-in function templates with the kernels' parameter lists record the tuple they were instantiated
//   with: k_apply (3 formats x alpha x chunked x {replace, dither, dither with a map} = 36), k_dither_lists (3 formats x halves x
//   alpha x {the reference's matrix, a map} = 24), diffusion (route x alpha x format x skew = 36).
#include <cstdint>
#include <cstdio>
#include <set>
#include <tuple>
#include <type_traits>

#include "kmg_dispatch.h"

using namespace kmg;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { ++failures; std::printf("line %d: %s\n", __LINE__, #cond); } } while (0)

// the output type as the format that selects it
template <typename T> constexpr int format_of() { return std::is_same<T, uint32_t>::value ? 0 : std::is_same<T, uint8_t>::value ? 1 : std::is_same<T, uint16_t>::value ? 2 : -1; }

typedef std::tuple<int, int, int, int> Tuple;

// the offsets types of the dither kernels (kmg_kernels.h), as the launchers choose between them
struct BayerOffsets {};
struct MapOffsets {};
template <class Off> constexpr int map_of() { return std::is_same<Off, MapOffsets>::value ? 1 : std::is_same<Off, BayerOffsets>::value ? 0 : -1; }

// stand-ins with the kernels' template parameter lists
template <int PPT, bool D, bool C, bool A, class OutT, class Off> static Tuple apply_standin()
{
    static_assert(PPT == 8, "");
    static_assert(D || map_of<Off>() == 0, "a map implies dither");
    return Tuple(D + map_of<Off>(), C, A, format_of<OutT>());         // 0 replace, 1 dither, 2 dither with a map
}
template <int H, bool A, class OutT, class Off> static Tuple lists_standin() { return Tuple(H, A, format_of<OutT>(), map_of<Off>()); }
template <int R, bool A, class OutT, int S> static Tuple diffuse_standin() { return Tuple(R, A, format_of<OutT>(), S); }

static void helpers()
{
    for (int b = 0; b < 2; ++b) {
        int calls = 0;
        const bool ran = with_bool(b != 0, [&](auto B) { ++calls; CHECK(decltype(B)::value == (b != 0)); CHECK(B() == (b != 0)); });
        CHECK(ran && calls == 1);
    }
    for (int format = -3; format <= 6; ++format) {
        int calls = 0;
        const bool ran = with_out_type(format, [&](auto t) { ++calls; CHECK(format_of<typename decltype(t)::type>() == format); });
        CHECK(ran == (format >= 0 && format <= 2) && calls == (ran ? 1 : 0));
        calls = 0;
        const bool ran_index = with_index_type(format, [&](auto t) {
            ++calls;
            CHECK(format_of<typename decltype(t)::type>() == format);
            CHECK(sizeof(typename decltype(t)::type) == (size_t)format);
        });
        CHECK(ran_index == (format == 1 || format == 2) && calls == (ran_index ? 1 : 0));
    }
    for (int wide = 0; wide < 2; ++wide) {
        int calls = 0;
        const bool ran = with_index_type(wide != 0, [&](auto t) { ++calls; CHECK(sizeof(typename decltype(t)::type) == (wide ? 2u : 1u)); });
        CHECK(ran && calls == 1);
    }
    // the integer sets of the launchers: PPT, list halves, skew, the error forms, the `what` masks, the packed widths
    auto value_set = [](auto with, std::set<int> listed) {
        for (int v = -2; v <= 20; ++v) {
            int calls = 0;
            const bool ran = with(v, [&](auto V) { ++calls; CHECK(decltype(V)::value == v); CHECK(V() == v); });
            CHECK(ran == (listed.count(v) == 1) && calls == (ran ? 1 : 0));
        }
    };
    value_set([](int v, auto f) { return with_value<1, 2, 4, 8>(v, f); }, {1, 2, 4, 8});
    value_set([](int v, auto f) { return with_value<1, 2>(v, f); }, {1, 2});
    value_set([](int v, auto f) { return with_value<2, 3>(v, f); }, {2, 3});
    value_set([](int v, auto f) { return with_value<1, 2, 3>(v, f); }, {1, 2, 3});
    value_set([](int v, auto f) { return with_value<0, 1, 2, 3>(v, f); }, {0, 1, 2, 3});
    value_set([](int v, auto f) { return with_value<1, 2, 4, 8, 16>(v, f); }, {1, 2, 4, 8, 16});
    value_set([](int v, auto f) { return with_value<7>(v, f); }, {7});
}

static void nests()
{
    // launch_apply (kmg_kernels.hip)
    std::set<Tuple> seen;
    int calls = 0;
    for (int format = 0; format < 3; ++format)
        for (int alpha = 0; alpha < 2; ++alpha)
            for (int pass = 0; pass < 3; ++pass)                       // replace, dither, dither with a map
                for (int chunked = 0; chunked < 2; ++chunked) {
                    const bool dither = pass != 0, map = pass == 2;
                    const bool known = with_out_type(format, [&](auto t) {
                        using OutT = typename decltype(t)::type;
                        with_value<0, 1, 2>(map ? 2 : dither ? 1 : 0, [&](auto D) { with_bool(chunked != 0, [&](auto C) { with_bool(alpha != 0, [&](auto A) {
                            using Off = std::conditional_t<D() == 2, MapOffsets, BayerOffsets>;
                            const Tuple got = apply_standin<8, D() != 0, C(), A(), OutT, Off>();
                            ++calls;
                            CHECK(got == Tuple(pass, chunked, alpha, format));
                            seen.insert(got);
                        }); }); });
                    });
                    CHECK(known);
                }
    CHECK(calls == 36 && seen.size() == 36);
    CHECK(!with_out_type(3, [&](auto) { ++calls; }) && calls == 36);

    // launch_dither_lists (kmg_lists.hip)
    seen.clear();
    calls = 0;
    for (int format = 0; format < 3; ++format)
        for (int halves = 1; halves <= 2; ++halves)
            for (int alpha = 0; alpha < 2; ++alpha)
                for (int map = 0; map < 2; ++map) {
                    const bool known = with_out_type(format, [&](auto t) {
                        using OutT = typename decltype(t)::type;
                        with_value<1, 2>(halves, [&](auto H) { with_bool(alpha != 0, [&](auto A) { with_bool(map != 0, [&](auto M) {
                            using Off = std::conditional_t<M(), MapOffsets, BayerOffsets>;
                            const Tuple got = lists_standin<H(), A(), OutT, Off>();
                            ++calls;
                            CHECK(got == Tuple(halves, alpha, format, map));
                            seen.insert(got);
                        }); }); });
                    });
                    CHECK(known);
                }
    CHECK(calls == 24 && seen.size() == 24);

    // launch_diffuse_wide (kmg_diffuse_wide.hip); launch_diffuse is the same nest without the skew.  An input outside the sets
    // launches nothing.
    seen.clear();
    calls = 0;
    for (int route = -1; route <= 3; ++route)
        for (int alpha = 0; alpha < 2; ++alpha)
            for (int format = -1; format <= 3; ++format)
                for (int skew = 1; skew <= 4; ++skew) {
                    bool launched = false;
                    with_value<0, 1, 2>(route, [&](auto R) { with_bool(alpha != 0, [&](auto A) {
                        with_out_type(format, [&](auto t) { with_value<2, 3>(skew, [&](auto S) {
                            using OutT = typename decltype(t)::type;
                            const Tuple got = diffuse_standin<R(), A(), OutT, S()>();
                            ++calls;
                            launched = true;
                            CHECK(got == Tuple(route, alpha, format, skew));
                            seen.insert(got);
                        }); });
                    }); });
                    CHECK(launched == (route >= 0 && route <= 2 && format >= 0 && format <= 2 && (skew == 2 || skew == 3)));
                }
    CHECK(calls == 36 && seen.size() == 36);
}

int main()
{
    helpers();
    nests();
    std::printf("dispatch ok: failures %d\n", failures);
    return failures ? 1 : 0;
}
