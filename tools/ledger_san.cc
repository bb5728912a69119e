// ledger_san.cc -- a stand-alone driver of the planner's assume ledger through
// the JSON ABI (include/jsk_host.h) with no engine bound, for an ASan + UBSan
// build of the host mirror (`make tools/bin/ledger_san`): the placing methods'
// request front (each ends at "no engine bound"), assume, a repeated assume, a
// sync that confirms one job, forget, a structural change and a rack that
// disappears. Host code only; no GPU is touched (planner.new engine 0).
// Exit status 0 when every reply carries the expected counts.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../include/jsk_host.h"

static int g_bad = 0;

// want_error null: the reply must carry no "error"; else it must carry this text
static std::string call(const char* method, const std::string& req, const char* want_error = nullptr) {
    char* out = nullptr;
    const int rc = jsk_call(method, req.c_str(), &out);
    std::string r = out ? out : "";
    jsk_free(out);
    const bool ok = want_error ? r.find(std::string("\"error\":\"") + want_error + "\"") != std::string::npos
                               : r.find("\"error\"") == std::string::npos;
    if (rc != 0 || !ok) {
        std::fprintf(stderr, "%s: rc=%d %s\n", method, rc, r.c_str());
        ++g_bad;
    }
    return r;
}

// the integer behind the first "key": of a reply (-1: absent)
static long num(const std::string& r, const char* key) {
    const std::string k = std::string("\"") + key + "\"";
    size_t i = r.find(k);
    if (i == std::string::npos) return -1;
    i = r.find(':', i + k.size());
    if (i == std::string::npos) return -1;
    return std::strtol(r.c_str() + i + 1, nullptr, 10);
}

static void expect(const char* what, long got, long want) {
    if (got != want) {
        std::fprintf(stderr, "%s: got %ld, want %ld\n", what, got, want);
        ++g_bad;
    }
}

static std::string node(int z, int r, int n) {
    char b[512];
    std::snprintf(b, sizeof b,
                  "{\"metadata\":{\"name\":\"z%d-r%d-n%d\",\"labels\":{\"zone\":\"zone-%d\",\"rack\":\"zone-%d-rack-%d\"}},"
                  "\"spec\":{\"taints\":[]},\"status\":{\"allocatable\":{\"amd.com/gpu\":\"8\"}}}",
                  z, r, n, z, z, r);
    return b;
}

static std::string job(const char* name) {
    char b[1024];
    std::snprintf(b, sizeof b,
                  "{\"metadata\":{\"name\":\"%s\",\"namespace\":\"default\","
                  "\"labels\":{\"jobset.sigs.k8s.io/replicatedjob-name\":\"workers\",\"jobset.sigs.k8s.io/job-key\":\"key-%s\"},"
                  "\"annotations\":{\"alpha.jobset.sigs.k8s.io/exclusive-topology\":\"rack\"}},"
                  "\"spec\":{\"parallelism\":2,\"template\":{\"spec\":{\"containers\":[{\"name\":\"c\","
                  "\"resources\":{\"requests\":{\"amd.com/gpu\":\"8\"}}}]}}}}",
                  name, name);
    return b;
}

int main() {
    const std::string made = call("cache.new", "{}");
    const std::string id = std::to_string(num(made, "result"));
    const std::string c = "\"cache\":" + id;
    call("planner.new", "{" + c + ",\"engine\":0,\"levelKeys\":[\"zone\",\"rack\"],\"resources\":[\"amd.com/gpu\"]}");
    for (int z = 0; z < 2; ++z)
        for (int r = 0; r < 2; ++r)
            for (int n = 0; n < 2; ++n)
                call("cache.add", "{" + c + ",\"kind\":\"Node\",\"object\":" + node(z, r, n) + "}");
    expect("rows", num(call("planner.sync", "{" + c + "}"), "rows"), 8);
    const std::string jobs = "\"jobs\":[" + job("a") + "," + job("b") + "," + job("c") + "]";
    const std::string where =
        "\"assignment\":{\"a\":\"zone-0-rack-1\",\"b\":\"zone-1-rack-0\",\"c\":\"zone-9-rack-9\"}";
    // the placing methods' request front, engine-less: everything up to the engine call runs
    const char* const no_engine = "planner: no engine bound";
    std::string r = call("planner.encode", "{" + c + "," + jobs + "}");
    expect("encoded pods", num(r, "pods"), 2);
    call("planner.plan", "{" + c + "," + jobs + ",\"previous\":{\"a\":\"zone-0-rack-1\",\"c\":\"zone-9-rack-9\"}}", no_engine);
    call("planner.explain", "{" + c + "," + jobs + "}", no_engine);
    call("planner.planGangs", "{" + c + "," + jobs + ",\"spans\":{\"default/\":\"zone\"}}", no_engine);
    call("planner.planFit", "{" + c + "," + jobs + ",\"policy\":\"tightest\"}", no_engine);
    call("planner.bind", "{" + c + "," + jobs + "," + where + "}", no_engine);
    r = call("planner.assume", "{" + c + "," + jobs + "," + where + "}");
    expect("committed", num(r, "rowsMarked"), 4);
    expect("assumed", num(r, "assumed"), 2);
    r = call("planner.assume", "{" + c + "," + jobs + "," + where + "}");  // held already: stale, the ledger as it was
    expect("stale", num(r, "stale"), 2);
    expect("assumed again", num(r, "assumed"), 2);
    // job a's leader pod shows up: the sync confirms it and drops the entry
    call("cache.add", "{" + c + ",\"kind\":\"Pod\",\"object\":{\"metadata\":{\"name\":\"a-0\",\"namespace\":\"default\","
                      "\"labels\":{\"jobset.sigs.k8s.io/job-key\":\"key-a\"},"
                      "\"annotations\":{\"alpha.jobset.sigs.k8s.io/exclusive-topology\":\"rack\"}},"
                      "\"spec\":{\"nodeName\":\"z0-r1-n0\",\"containers\":[{\"name\":\"c\"}]},"
                      "\"status\":{\"phase\":\"Running\"}}}");
    expect("exclusiveJobs", num(call("planner.sync", "{" + c + "}"), "exclusiveJobs"), 1);
    r = call("planner.forget", "{" + c + ",\"jobs\":[\"a\",\"nobody\"]}");
    expect("confirmed job: rowsCleared", num(r, "rowsCleared"), 0);
    expect("confirmed job: assumed", num(r, "assumed"), 1);
    // a structural change keeps job b's hold; the columns still carry its owner
    call("cache.add", "{" + c + ",\"kind\":\"Node\",\"object\":" + node(1, 1, 2) + "}");
    expect("rows after a node joined", num(call("planner.sync", "{" + c + "}"), "rows"), 9);
    r = call("planner.columns", "{" + c + "}");
    if (r.find("1073741825") == std::string::npos) {  // 0x40000001: job b's owner
        std::fprintf(stderr, "job b's owner left the columns: %s\n", r.c_str());
        ++g_bad;
    }
    r = call("planner.forget", "{" + c + ",\"jobs\":[\"b\"]}");
    expect("rowsCleared", num(r, "rowsCleared"), 2);
    expect("assumed after forget", num(r, "assumed"), 0);
    // a hold whose rack disappears goes with it
    r = call("planner.assume", "{" + c + "," + jobs + "," + where + "}");
    expect("assumed once more", num(r, "assumed"), 1);  // job a's rack belongs to the informer now: stale
    call("cache.remove", "{" + c + ",\"kind\":\"Node\",\"name\":\"z1-r0-n0\"}");
    call("cache.remove", "{" + c + ",\"kind\":\"Node\",\"name\":\"z1-r0-n1\"}");
    call("planner.sync", "{" + c + "}");
    r = call("planner.forget", "{" + c + ",\"jobs\":[\"b\"]}");
    expect("rowsCleared of a vanished rack", num(r, "rowsCleared"), 0);
    expect("assumed at the end", num(r, "assumed"), 0);
    call("cache.free", "{" + c + "}");
    std::printf("ledger_san: %s\n", g_bad ? "FAILED" : "ok");
    return g_bad ? 1 : 0;
}
