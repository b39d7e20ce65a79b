// Stand-alone check of the kernel-switch table and parser of vqvdb_amd/csrc/vq_switches.h against a fake environment.  Built with
// -fsanitize=address,undefined by tests/test_switches_host.py; exits 0 when every check holds, prints the failed checks and exits 1
// otherwise.  With the argument `table` it prints the switches as the Markdown table that stands in INTEGRATION.md.
//
// The expectations below are written out by hand from the strcmp lines that vqhip_create held before the table existed; nothing in
// them is derived from the table under test except the list of names to walk.
#include <cctype>
#include <cstdio>
#include <functional>
#include <map>
#include <string>
#include <vector>

#include "../../vqvdb_amd/csrc/vq_switches.h"

namespace {

constexpr int DEVICE_CUS = 256;

std::map<std::string, std::string> g_env;
const char* fake_lookup(const char* name)
{
    auto it = g_env.find(name);
    return it == g_env.end() ? nullptr : it->second.c_str();
}

int failures = 0;
void fail(const std::string& what)
{
    std::printf("FAILED: %s\n", what.c_str());
    ++failures;
}

// the defaults of a handle on a device with DEVICE_CUS compute units, field by field
Switches defaults()
{
    Switches d;
    d.n_cus = DEVICE_CUS;
    d.stem_fused = true, d.stem_taps = true, d.stem_small_fused = true;
    d.tail_groups = false, d.tail_rows32 = false, d.tail_rows = true;
    d.host_split = 8, d.host_split_min = 8192;
    d.tail16_tiles = 48;
    d.r64s_resident = true;
    d.vq_split = 2;
    d.conv8_w16 = true, d.conv8_lds = true, d.convdown_lds = true, d.conv4_lds = true;
    d.first_once = true, d.first_roll_stats = false, d.first_raw = false, d.first_roll = true;
    d.train_gn_fused = true;
    d.train_bias_main = true, d.train_red_stream = false, d.train_red_deferred = true;
    d.train_ema_early = true;
    d.train_side_stream = true, d.train_side_prio = 0;
    d.train_red_queue_mask = true, d.train_red_prio = 0, d.train_red_own_leaves = 2048;
    d.train_r64_quarters = true, d.train_dgrad_small_lds = true;
    d.train_wgrad_cu_pct = 100;
    d.train_wgrad_rows = true, d.train_stem_lut = true, d.train_ema_lists = true, d.train_folded_tail = true;
    return d;
}

// every field by name, so that a mismatch says which one
#define FIELDS(F)                                                                                                                    \
    F(n_cus) F(stem_fused) F(stem_taps) F(stem_small_fused) F(tail_groups) F(tail_rows32) F(tail_rows) F(host_split) F(host_split_min) \
    F(tail16_tiles) F(r64s_resident) F(vq_split) F(conv8_w16) F(convdown_lds) F(conv4_lds) F(first_once) F(first_roll_stats)         \
    F(first_raw) F(first_roll) F(conv8_lds) F(train_gn_fused) F(train_bias_main) F(train_red_stream) F(train_red_deferred)           \
    F(train_ema_early) F(train_side_stream) F(train_side_prio) F(train_red_queue_mask) F(train_red_prio) F(train_red_own_leaves)     \
    F(train_r64_quarters) F(train_dgrad_small_lds) F(train_wgrad_cu_pct) F(train_wgrad_rows) F(train_stem_lut) F(train_ema_lists)    \
    F(train_folded_tail)

std::string difference(const Switches& got, const Switches& want)
{
    std::string d;
#define F(f) \
    if (got.f != want.f) d += std::string(" " #f "=") + std::to_string((long long)got.f) + " (want " + std::to_string((long long)want.f) + ")";
    FIELDS(F)
#undef F
    return d;
}

// A struct that no parse can produce: every field differs from every value the table can give.  parse_switches must leave it alone
// when it fails.
Switches poisoned()
{
    Switches p;
#define F(f) p.f = (decltype(p.f))77;
    FIELDS(F)
#undef F
    p.n_cus = -7, p.host_split = -7, p.host_split_min = -7, p.tail16_tiles = -7, p.vq_split = -7, p.train_wgrad_cu_pct = -7, p.train_red_own_leaves = -7;
    p.train_side_prio = 7, p.train_red_prio = 7;
    return p;
}

struct Outcome {
    int rc;
    Switches s;
    std::string err;
};
Outcome parse(const std::map<std::string, std::string>& env, const Switches& start)
{
    g_env = env;
    Outcome o{0, start, ""};
    o.rc = parse_switches(o.s, fake_lookup, DEVICE_CUS, o.err);
    return o;
}

void expect_ok(const std::map<std::string, std::string>& env, const Switches& want, const std::string& label)
{
    const Outcome o = parse(env, poisoned());   // (a successful parse starts from the defaults, whatever the struct held)
    if (o.rc != VQHIP_OK) return fail(label + ": refused: " + o.err);
    const std::string d = difference(o.s, want);
    if (!d.empty()) fail(label + ":" + d);
}

void expect_refused(const std::string& name, const std::string& value)
{
    const std::string label = name + "=" + value;
    const Outcome o = parse({{name, value}}, poisoned());
    if (o.rc != VQHIP_ERR_INVALID) return fail(label + ": rc " + std::to_string(o.rc) + ", want VQHIP_ERR_INVALID");
    if (o.err.find(name) == std::string::npos || o.err.find(value) == std::string::npos) fail(label + ": message lacks the switch or the value: " + o.err);
    if (o.err.compare(0, name.size() + 1, name + "=") != 0) fail(label + ": message does not begin with the switch's name: " + o.err);
    const std::string d = difference(o.s, poisoned());
    if (!d.empty()) fail(label + ": a refused parse changed the struct:" + d);
}

using Edit = std::function<void(Switches&)>;
struct Value {
    std::string word;
    Edit edit;   // what the word changes in the defaults
};
const Edit nothing = [](Switches&) {};

// enumerated switches: every legal word, the default's name first
const std::vector<std::pair<std::string, std::vector<Value>>> ENUMERATED = {
    {"VQHIP_CONV8", {{"w16", nothing}, {"w8", [](Switches& s) { s.conv8_w16 = false; }}, {"rows", [](Switches& s) { s.conv8_lds = false; }}}},
    {"VQHIP_CONV4", {{"lds", nothing}, {"rows", [](Switches& s) { s.conv4_lds = false; }}}},
    {"VQHIP_DOWN", {{"lds", nothing}, {"rows", [](Switches& s) { s.convdown_lds = false; }}}},
    {"VQHIP_FIRST",
     {{"once", nothing},
      {"twopass", [](Switches& s) { s.first_once = false; }},
      {"steps", [](Switches& s) { s.first_once = false, s.first_roll = false; }},
      {"roll0", [](Switches& s) { s.first_once = false, s.first_roll_stats = true; }}}},
    {"VQHIP_FIRST_SRC", {{"packed", nothing}, {"raw", [](Switches& s) { s.first_raw = true; }}}},
    {"VQHIP_STEM", {{"taps", nothing}, {"gather", [](Switches& s) { s.stem_taps = false; }}, {"split", [](Switches& s) { s.stem_fused = false; }}}},
    {"VQHIP_STEM_SMALL", {{"fused", nothing}, {"split", [](Switches& s) { s.stem_small_fused = false; }}}},
    {"VQHIP_TAIL",
     {{"rows16", nothing},
      {"rows32", [](Switches& s) { s.tail_rows32 = true; }},
      {"groups", [](Switches& s) { s.tail_groups = true; }},
      {"slab", [](Switches& s) { s.tail_rows = false; }}}},
    {"VQHIP_R64S", {{"resident", nothing}, {"stream", [](Switches& s) { s.r64s_resident = false; }}}},
    {"VQHIP_TRAIN_STEM", {{"lut", nothing}, {"conv", [](Switches& s) { s.train_stem_lut = false; }}}},
    {"VQHIP_TRAIN_WGRAD", {{"rows", nothing}, {"pairs", [](Switches& s) { s.train_wgrad_rows = false; }}}},
    {"VQHIP_TRAIN_STREAMS", {{"2", nothing}, {"1", [](Switches& s) { s.train_side_stream = false; }}}},
    {"VQHIP_TRAIN_GNBWD", {{"fused", nothing}, {"split", [](Switches& s) { s.train_gn_fused = false; }}}},
    {"VQHIP_TRAIN_BIAS",   // (train_bias_main, train_red_stream, train_red_deferred)
     {{"deferred", [](Switches& s) { s.train_bias_main = true, s.train_red_stream = false, s.train_red_deferred = true; }},
      {"main", [](Switches& s) { s.train_bias_main = true, s.train_red_stream = false, s.train_red_deferred = false; }},
      {"side", [](Switches& s) { s.train_bias_main = false, s.train_red_stream = false, s.train_red_deferred = false; }},
      {"third", [](Switches& s) { s.train_bias_main = true, s.train_red_stream = true, s.train_red_deferred = false; }}}},
    {"VQHIP_TRAIN_R64", {{"quarters", nothing}, {"whole", [](Switches& s) { s.train_r64_quarters = false; }}}},
    {"VQHIP_TRAIN_DGRAD", {{"streamed", nothing}, {"resident", [](Switches& s) { s.train_dgrad_small_lds = false; }}}},
    {"VQHIP_TRAIN_EMA_AT", {{"forward", nothing}, {"backward", [](Switches& s) { s.train_ema_early = false; }}}},
    {"VQHIP_TRAIN_EMA", {{"lists", nothing}, {"scan", [](Switches& s) { s.train_ema_lists = false; }}}},
    {"VQHIP_TRAIN_TAIL", {{"folded", nothing}, {"unfolded", [](Switches& s) { s.train_folded_tail = false; }}}},
    {"VQHIP_TRAIN_SIDE_PRIO", {{"plain", nothing}, {"high", [](Switches& s) { s.train_side_prio = 1; }}, {"low", [](Switches& s) { s.train_side_prio = -1; }}}},
    {"VQHIP_TRAIN_RED_QUEUE", {{"mask", nothing}, {"prio", [](Switches& s) { s.train_red_queue_mask = false; }}}},
    {"VQHIP_TRAIN_RED_PRIO", {{"auto", nothing}, {"own", [](Switches& s) { s.train_red_prio = 1; }}, {"normal", [](Switches& s) { s.train_red_prio = -1; }}}},
};

// integer switches: the range (max < 0: none), a legal value and the field it lands in
struct Integer {
    std::string name;
    long lo, hi;
    long legal;
    std::function<void(Switches&, long)> edit;
};
const std::vector<Integer> INTEGERS = {
    {"VQHIP_CUS", 1, DEVICE_CUS, 3, [](Switches& s, long v) { s.n_cus = (int)v; }},
    {"VQHIP_TAIL16_TILES", 0, 2147483647L, 0, [](Switches& s, long v) { s.tail16_tiles = (int)v; }},
    {"VQHIP_VQ_SPLIT", 1, 64, 64, [](Switches& s, long v) { s.vq_split = (int)v; }},
    {"VQHIP_HOST_SPLIT", 1, 2147483647L, 3, [](Switches& s, long v) { s.host_split = (int)v; }},
    {"VQHIP_TRAIN_WGRAD_CU_PCT", 10, 100, 10, [](Switches& s, long v) { s.train_wgrad_cu_pct = (int)v; }},
    {"VQHIP_TRAIN_RED_OWN_LEAVES", 0, -1, 4096, [](Switches& s, long v) { s.train_red_own_leaves = v; }},
    {"VQHIP_COPY_THREADS", 1, 2147483647L, 4, [](Switches&, long) {}},   // process-wide: validated at create, held by copy_threads_cap()
};

void check_everything()
{
    const Switches D = defaults();
    expect_ok({}, D, "no variable set");
    {   // the defaults of the struct itself (what a handle holds before create has parsed anything) differ in nothing but n_cus
        Switches fresh;
        fresh.n_cus = DEVICE_CUS;
        const std::string d = difference(fresh, D);
        if (!d.empty()) fail("Switches{}:" + d);
    }

    size_t walked = 0;
    for (const auto& sw : ENUMERATED) {
        const std::string& name = sw.first;
        ++walked;
        for (const Value& v : sw.second) {
            Switches want = D;
            v.edit(want);
            expect_ok({{name, v.word}}, want, name + "=" + v.word);
        }
        expect_ok({{name, ""}}, D, name + " empty");
        // a typo: the first non-default word without its last letter.  (VQHIP_TRAIN_STREAMS' "1" would become the empty string, which
        // means the default by definition: a one-letter word is doubled instead.)  Then trailing / leading space and upper case.
        const std::string& word = sw.second[1].word;
        expect_refused(name, word.size() > 1 ? word.substr(0, word.size() - 1) : word + word);
        expect_refused(name, word + " ");
        expect_refused(name, " " + word);
        std::string upper = word;
        for (char& ch : upper) ch = (char)std::toupper((unsigned char)ch);
        if (upper != word) expect_refused(name, upper);
    }
    for (const Integer& sw : INTEGERS) {
        ++walked;
        Switches want = D;
        sw.edit(want, sw.legal);
        expect_ok({{sw.name, std::to_string(sw.legal)}}, want, sw.name + "=" + std::to_string(sw.legal));
        want = D, sw.edit(want, sw.lo);
        expect_ok({{sw.name, std::to_string(sw.lo)}}, want, sw.name + " at its minimum");
        if (sw.hi >= 0) {
            want = D, sw.edit(want, sw.hi);
            expect_ok({{sw.name, std::to_string(sw.hi)}}, want, sw.name + " at its maximum");
            expect_refused(sw.name, std::to_string(sw.hi + 1));
        }
        expect_ok({{sw.name, ""}}, D, sw.name + " empty");
        for (const char* bad : {"abc", "4x", " 7", "99999999999999999999", "-99999999999999999999", "7 ", "0x10", "1e2", "-", "+"}) expect_refused(sw.name, bad);
        expect_refused(sw.name, std::to_string(sw.lo - 1));
    }
    if (walked != sizeof(vqsw::SWITCHES) / sizeof(vqsw::SWITCHES[0])) fail("the table holds " + std::to_string(sizeof(vqsw::SWITCHES) / sizeof(vqsw::SWITCHES[0])) + " switches, this program walks " + std::to_string(walked));
    for (const vqsw::Switch& w : vqsw::SWITCHES) {   // ... and the same ones
        bool known = false;
        for (const auto& sw : ENUMERATED) known = known || sw.first == w.name;
        for (const Integer& sw : INTEGERS) known = known || sw.name == w.name;
        if (!known) fail(std::string(w.name) + " is in the table and not in this program");
    }

    // VQHIP_CUS as before the table (tests/test_gpu_cu_counts.py::test_values_outside_the_range_are_refused_at_create)
    for (const std::string& bad : {std::string("0"), std::string("-1"), std::string("abc"), std::to_string(DEVICE_CUS + 1)}) {
        expect_refused("VQHIP_CUS", bad);
        const Outcome o = parse({{"VQHIP_CUS", bad}}, D);
        const std::string want = "VQHIP_CUS=" + bad + ": not an integer in [1, " + std::to_string(DEVICE_CUS) + "] (the device's compute units)";
        if (o.err != want) fail("VQHIP_CUS=" + bad + ": message '" + o.err + "', want '" + want + "'");
    }
    {
        const Outcome o = parse({{"VQHIP_TAIL", "rows"}}, D);
        if (o.err.find("rows16 | rows32 | groups | slab") == std::string::npos) fail("VQHIP_TAIL=rows: the message does not list the legal values: " + o.err);
    }

    // VQHIP_HOST_SPLIT = n or n,min
    {
        Switches want = D;
        want.host_split = 1;
        expect_ok({{"VQHIP_HOST_SPLIT", "1"}}, want, "VQHIP_HOST_SPLIT=1");
        want.host_split = 5, want.host_split_min = 4096;
        expect_ok({{"VQHIP_HOST_SPLIT", "5,4096"}}, want, "VQHIP_HOST_SPLIT=5,4096");
        want.host_split = 4, want.host_split_min = 32;
        expect_ok({{"VQHIP_HOST_SPLIT", "4,32"}}, want, "VQHIP_HOST_SPLIT=4,32");
        for (const char* bad : {"0", "4,31", "4,", ",32", "4,32,1", "4, 32", "4,abc", "0,32"}) expect_refused("VQHIP_HOST_SPLIT", bad);
    }

    // several at once, one of them wrong: refused, and the message names the wrong one
    {
        const Outcome o = parse({{"VQHIP_CONV8", "w8"}, {"VQHIP_TAIL", "slab"}, {"VQHIP_TRAIN_BIAS", "thrid"}}, poisoned());
        if (o.rc != VQHIP_ERR_INVALID || o.err.find("VQHIP_TRAIN_BIAS=thrid") != 0 || !difference(o.s, poisoned()).empty()) fail("one wrong value among three: " + o.err);
        Switches want = D;
        want.conv8_w16 = false, want.tail_rows = false, want.train_bias_main = true, want.train_red_stream = true, want.train_red_deferred = false;
        expect_ok({{"VQHIP_CONV8", "w8"}, {"VQHIP_TAIL", "slab"}, {"VQHIP_TRAIN_BIAS", "third"}}, want, "three at once");
    }
}

std::string cell(std::string text)   // '|' separates table cells
{
    for (size_t i = 0; (i = text.find('|', i)) != std::string::npos; i += 2) text.replace(i, 1, "\\|");
    return text;
}

void print_table()
{
    std::printf("| switch | values (default first) | selects | covered by |\n|---|---|---|---|\n");
    for (const vqsw::Switch& w : vqsw::SWITCHES) {
        std::string values = vqsw::legal_values(w), shown;
        if (w.is_integer()) shown = values;
        else
            for (const vqsw::Word& x : w.words)
                if (x.word) shown += (shown.empty() ? "`" : " \\| `") + std::string(x.word) + "`";
        std::printf("| `%s` | %s | %s | %s |\n", w.name, shown.c_str(), cell(w.selects).c_str(), *w.covered_by ? (std::string("`") + w.covered_by + "`").c_str() : "");
    }
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc == 2 && std::string(argv[1]) == "table") {
        print_table();
        return 0;
    }
    check_everything();
    if (failures) return 1;
    std::printf("switches ok: %zu switches\n", sizeof(vqsw::SWITCHES) / sizeof(vqsw::SWITCHES[0]));
    return 0;
}
