// pt_path_expr.cpp — the compiler of path expressions (include/pt_light_groups.h, "Path expressions"): host code alone, no HIP.
// pt_path_expr_compile parses every expression into a Thompson automaton over the three event symbols whose last node carries the expression's terminals, takes
// the union, determinises it by subsets, merges the states no continuation tells apart (Moore) and writes the table the kernels, the emulation and the tests
// read: 16 bytes per state, the successors in word 0 and nine 8-bit output masks in words 1..3.  pt_path_expr_match runs that table over a written-out path.
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../include/pt_light_groups.h"

namespace {

constexpr uint32_t kEvents = 3;       // D, R, T: PP_DIFFUSE, PP_REFLECTION, PP_TRANSMISSION of pt_path_pass_rules.h
constexpr uint32_t kTerminals = PT_PATH_EXPR_TERMINALS;
constexpr size_t kSubsetLimit = 1u << 16;   // subsets made before the determinisation gives up counting

struct Node {
    std::vector<uint32_t> eps;
    uint32_t symbols = 0, target = 0;   // one labelled edge at most: the events of `symbols` (bit per event) lead to `target`
    uint32_t terminals = 0, expr = 0;   // an alternative's last node: bit per terminal symbol it accepts, for expression `expr`
};
struct Fragment { uint32_t first, last; };

struct SyntaxError { size_t column; std::string what; };

int event_of(char c) { return c == 'D' ? 0 : c == 'R' ? 1 : c == 'T' ? 2 : -1; }

// One expression's text -> nodes of the shared automaton.  Columns count from 1 in the text as given; white space is skipped wherever a symbol is looked for.
struct Parser {
    const char* text;
    size_t at = 0;
    uint32_t expr, environment_group;
    std::vector<Node>& nodes;

    Parser(const char* t, uint32_t e, uint32_t env, std::vector<Node>& n) : text(t), expr(e), environment_group(env), nodes(n) {}

    [[noreturn]] void fail(const std::string& what) { throw SyntaxError{at + 1, what}; }
    char peek() {
        while (text[at] == ' ' || text[at] == '\t' || text[at] == '\n' || text[at] == '\r') ++at;
        return text[at];
    }
    char take() { const char c = peek(); ++at; return c; }
    uint32_t node() { nodes.emplace_back(); return (uint32_t)nodes.size() - 1u; }
    Fragment edge(uint32_t symbols) {
        const uint32_t a = node(), b = node();
        nodes[a].symbols = symbols; nodes[a].target = b;
        return Fragment{a, b};
    }
    bool terminal_ahead() {   // L, E, or a class that begins with one of them
        const char c = peek();
        if (c == 'L' || c == 'E') return true;
        if (c != '[') return false;
        const size_t keep = at;
        ++at;
        const char d = peek();
        at = keep;
        return d == 'L' || d == 'E';
    }
    // L, L<g>, E, E<g>: the terminal symbols it names
    uint32_t terminal_item() {
        const char c = take();
        const char d = text[at];   // (a digit belongs to its letter: no white space between them)
        const bool digit = d >= '0' && d <= '9';
        if (digit && d > '7') fail(std::string("light group ") + d + ": the groups are 0..7");
        if (digit) ++at;
        if (c == 'L') return digit ? 1u << (uint32_t)(d - '0') : 0xffu;
        return (!digit || (uint32_t)(d - '0') == environment_group) ? 1u << PT_PATH_EXPR_ENVIRONMENT : 0u;
    }
    uint32_t terminal() {
        if (peek() != '[') return terminal_item();
        take();
        uint32_t set = 0;
        for (;;) {
            const char c = peek();
            if (c == ']') { take(); return set; }
            if (c != 'L' && c != 'E') fail(c ? std::string("'") + c + "' in a class of terminals" : std::string("the class of terminals is not closed"));
            set |= terminal_item();
        }
    }
    Fragment atom() {
        const char c = peek();
        if (event_of(c) >= 0) { take(); return edge(1u << event_of(c)); }
        if (c == '.') { take(); return edge(7u); }
        if (c == '[') {
            take();
            bool negate = false;
            if (peek() == '^') { take(); negate = true; }
            uint32_t set = 0;
            for (;;) {
                const char d = peek();
                if (d == ']') { take(); break; }
                if (event_of(d) < 0) fail(d ? std::string("'") + d + "' in a class of events" : std::string("the class of events is not closed"));
                take();
                set |= 1u << event_of(d);
            }
            if (negate) set = ~set & 7u;
            if (set == 0) { --at; fail("the class of events is empty"); }
            return edge(set);
        }
        if (c == '(') {
            take();
            const Fragment f = alternatives(true);
            if (peek() != ')') fail("')' expected");
            take();
            return f;
        }
        if (c == '*' || c == '+' || c == '?') fail(std::string("'") + c + "' follows no event");
        if (c == 'C') fail("C stands only at the start of an alternative");
        if (c == 0) fail("the expression ends without a terminal (L, E, L0..L7, E0..E7 or a class of them)");
        fail(std::string("'") + c + "' is no part of a path expression");
    }
    Fragment repeated() {
        Fragment f = atom();
        for (;;) {
            const char c = peek();
            if (c != '*' && c != '+' && c != '?') return f;
            take();
            const uint32_t a = node(), b = node();
            nodes[a].eps.push_back(f.first); nodes[f.last].eps.push_back(b);
            if (c != '+') nodes[a].eps.push_back(b);
            if (c != '?') nodes[f.last].eps.push_back(f.first);
            f = Fragment{a, b};
        }
    }
    // events in a row, up to what ends them: ')' or '|', a terminal, the end of the text
    Fragment sequence(bool grouped) {
        const uint32_t a = node();
        Fragment f{a, a};
        for (;;) {
            const char c = peek();
            if (c == ')' || c == '|' || c == 0) break;
            if (terminal_ahead()) { if (grouped) fail("a terminal inside a group: every alternative ends in exactly one, at its end"); break; }
            const Fragment g = repeated();
            nodes[f.last].eps.push_back(g.first);
            f.last = g.last;
        }
        return f;
    }
    Fragment alternatives(bool grouped) {
        if (peek() == ')') fail("an empty group");
        const uint32_t a = node(), b = node();
        for (;;) {
            const Fragment f = sequence(grouped);
            nodes[a].eps.push_back(f.first); nodes[f.last].eps.push_back(b);
            if (peek() != '|') break;
            take();
        }
        return Fragment{a, b};
    }
    // C events terminal ( | C events terminal )*: the first nodes of the alternatives
    void expression(std::vector<uint32_t>* firsts) {
        for (;;) {
            if (peek() != 'C') fail(peek() ? "every alternative starts with C, the camera" : "the expression is empty: every alternative starts with C, the camera");
            take();
            const Fragment f = sequence(false);
            if (peek() == ')') fail("')' closes no group");
            if (!terminal_ahead()) {
                if (peek() == '|') fail("'|' where the alternative's terminal should stand (an alternation of events goes in a group)");
                fail("the expression ends without a terminal (L, E, L0..L7, E0..E7 or a class of them)");
            }
            nodes[f.last].terminals = terminal();
            nodes[f.last].expr = expr;
            firsts->push_back(f.first);
            const char c = peek();
            if (c == 0) return;
            if (c != '|') fail("an alternative ends with its terminal: only '|' and another alternative may follow");
            take();
        }
    }
};

void closure(const std::vector<Node>& nodes, std::vector<uint32_t>* set) {
    std::vector<bool> in(nodes.size(), false);
    std::vector<uint32_t> todo = *set;
    for (uint32_t n : todo) in[n] = true;
    while (!todo.empty()) {
        const uint32_t n = todo.back();
        todo.pop_back();
        for (uint32_t m : nodes[n].eps) if (!in[m]) { in[m] = true; todo.push_back(m); }
    }
    set->clear();
    for (uint32_t n = 0; n < nodes.size(); ++n) if (in[n]) set->push_back(n);
}

struct State { uint32_t next[kEvents]; uint8_t mask[kTerminals]; };

void put_error(char* err, size_t err_len, const std::string& what) {
    if (err && err_len) snprintf(err, err_len, "%s", what.c_str());
}

bool program_is_sound(const pt_path_expr_program* p) {
    if (!p || p->outputs == 0 || p->outputs > PT_PATH_EXPRS_MAX || p->states == 0 || p->states > PT_PATH_EXPR_STATES_MAX || p->start >= p->states) return false;
    for (uint32_t q = 0; q < p->states; ++q)
        for (uint32_t e = 0; e < kEvents; ++e) if (((p->table[q][0] >> (6u * e)) & 63u) >= p->states) return false;
    return true;
}

}  // namespace

extern "C" {

pt_status pt_path_expr_compile(const char* const* exprs, uint32_t n, uint32_t environment_group, pt_path_expr_program* program, char* err, size_t err_len) {
    put_error(err, err_len, "");
    if (!exprs || !program) { put_error(err, err_len, "the expressions or the program is null"); return PT_ERR_INVALID_ARGUMENT; }
    if (n == 0 || n > PT_PATH_EXPRS_MAX) { put_error(err, err_len, "the number of expressions must be in 1..8"); return PT_ERR_INVALID_ARGUMENT; }
    if (environment_group >= PT_LIGHT_GROUPS_MAX) { put_error(err, err_len, "environment_group must be below 8"); return PT_ERR_INVALID_ARGUMENT; }
    std::vector<Node> nodes;
    std::vector<uint32_t> firsts;
    for (uint32_t e = 0; e < n; ++e) {
        if (!exprs[e]) { put_error(err, err_len, "expression " + std::to_string(e) + " is null"); return PT_ERR_INVALID_ARGUMENT; }
        try {
            Parser(exprs[e], e, environment_group, nodes).expression(&firsts);
        } catch (const SyntaxError& s) {
            put_error(err, err_len, "expression " + std::to_string(e) + ", column " + std::to_string(s.column) + ": " + s.what);
            return PT_ERR_INVALID_ARGUMENT;
        }
    }
    // the subsets, in the order they are met from the start
    std::map<std::vector<uint32_t>, uint32_t> index;
    std::vector<std::vector<uint32_t>> subsets;
    std::vector<State> dfa;
    closure(nodes, &firsts);
    index[firsts] = 0u; subsets.push_back(firsts);
    for (size_t q = 0; q < subsets.size(); ++q) {
        State st;
        memset(&st, 0, sizeof(st));
        for (uint32_t m : subsets[q])
            for (uint32_t t = 0; t < kTerminals; ++t) if ((nodes[m].terminals >> t) & 1u) st.mask[t] |= (uint8_t)(1u << nodes[m].expr);
        for (uint32_t e = 0; e < kEvents; ++e) {
            std::vector<uint32_t> to;
            for (uint32_t m : subsets[q]) if ((nodes[m].symbols >> e) & 1u) to.push_back(nodes[m].target);
            closure(nodes, &to);
            auto found = index.find(to);
            if (found == index.end()) {
                if (subsets.size() >= kSubsetLimit) {
                    put_error(err, err_len, "the expressions determinise to more than " + std::to_string(kSubsetLimit) + " states; a program holds at most 64");
                    return PT_ERR_UNSUPPORTED;
                }
                found = index.emplace(to, (uint32_t)subsets.size()).first;
                subsets.push_back(to);
            }
            st.next[e] = found->second;
        }
        dfa.push_back(st);
    }
    // Moore: classes by the masks, split by the successors' classes until nothing splits; classes are numbered in the order their first state was met
    std::vector<uint32_t> cls(dfa.size(), 0u);
    size_t classes = 0;
    for (bool first = true;; first = false) {
        std::map<std::vector<uint32_t>, uint32_t> seen;
        std::vector<uint32_t> next_cls(dfa.size());
        for (size_t q = 0; q < dfa.size(); ++q) {
            std::vector<uint32_t> key;
            if (first) key.assign(dfa[q].mask, dfa[q].mask + kTerminals);
            else key = {cls[q], cls[dfa[q].next[0]], cls[dfa[q].next[1]], cls[dfa[q].next[2]]};
            next_cls[q] = seen.emplace(key, (uint32_t)seen.size()).first->second;
        }
        cls.swap(next_cls);
        if (!first && seen.size() == classes) break;
        classes = seen.size();
    }
    if (classes > PT_PATH_EXPR_STATES_MAX) {
        put_error(err, err_len, "the expressions need " + std::to_string(classes) + " states (" + std::to_string(dfa.size()) + " before minimisation); a program holds at most 64");
        return PT_ERR_UNSUPPORTED;
    }
    memset(program, 0, sizeof(*program));
    program->outputs = n; program->states = (uint32_t)classes; program->start = cls[0]; program->environment_group = environment_group;
    for (size_t q = 0; q < dfa.size(); ++q) {
        uint32_t* w = program->table[cls[q]];
        w[0] = cls[dfa[q].next[0]] | cls[dfa[q].next[1]] << 6 | cls[dfa[q].next[2]] << 12;
        w[1] = w[2] = w[3] = 0u;
        for (uint32_t t = 0; t < kTerminals; ++t) w[1u + t / 4u] |= (uint32_t)dfa[q].mask[t] << (8u * (t % 4u));
    }
    return PT_OK;
}

pt_status pt_path_expr_match(const pt_path_expr_program* program, const char* path, uint32_t* mask) {
    if (!program_is_sound(program) || !path || !mask) return PT_ERR_INVALID_ARGUMENT;
    *mask = 0u;
    const char* p = path;
    if (*p++ != 'C') return PT_ERR_INVALID_ARGUMENT;
    uint32_t q = program->start;
    for (; event_of(*p) >= 0; ++p) q = (program->table[q][0] >> (6u * (uint32_t)event_of(*p))) & 63u;
    if (*p != 'L' && *p != 'E') return PT_ERR_INVALID_ARGUMENT;
    const bool surface = *p++ == 'L';
    uint32_t group = surface ? 0u : program->environment_group;
    if (*p >= '0' && *p <= '7') group = (uint32_t)(*p++ - '0');
    if (*p != 0) return PT_ERR_INVALID_ARGUMENT;
    if (!surface && group != program->environment_group) return PT_OK;   // (the environment belongs to no other group: no such path)
    const uint32_t t = surface ? group : (uint32_t)PT_PATH_EXPR_ENVIRONMENT;
    *mask = (program->table[q][1u + t / 4u] >> (8u * (t % 4u))) & 0xffu;
    return PT_OK;
}

}  // extern "C"
