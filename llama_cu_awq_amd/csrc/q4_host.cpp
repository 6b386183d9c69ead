// q4_host.cpp -- host-only side of llama2_q4: the llama2.c BPE tokenizer (tokenizer.h), the generate / chat /
// perplexity drivers (llama2_q4.cu:436-601, perplexity.h:57-139) and the CLI (llama2_q4.cu:604-720).
// No device code here; everything reaches the GPU through the C ABI in llama2_q4.h, but for q4_loops.hip's token loop and the step it queues (q4_loop.h).
#include <ctype.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <string>
#include <vector>
#include "llama2_q4.h"
#include "q4_loop.h"

static const int bos_token = 1;   // tokenizer.h:8
static const int eos_token = 2;   // tokenizer.h:9

// ---------------------------------------------------------------------------------------------------
// Tokenizer (tokenizer.h:16-28). Lookup uses the same libc qsort/bsearch pair as the reference so that
// duplicate vocabulary strings (raw-byte pieces at ids 3..258) resolve to the same id.
struct TokenIndex {
    const char* str;
    int id;
};
struct Tokenizer {
    std::vector<std::string> vocab;
    std::vector<float> vocab_scores;
    std::vector<TokenIndex> sorted_vocab;   // built lazily by encode()
    int vocab_size;
    unsigned int max_token_length;
    unsigned char byte_pieces[512];
};

static int compare_tokens(const void* a, const void* b) {
    return strcmp(((const TokenIndex*)a)->str, ((const TokenIndex*)b)->str);
}

static int str_lookup(const char* str, Tokenizer* t) {                             // tokenizer.h:95-100
    TokenIndex tok = {str, 0};
    TokenIndex* res = (TokenIndex*)bsearch(&tok, t->sorted_vocab.data(), t->vocab_size, sizeof(TokenIndex), compare_tokens);
    return res != NULL ? res->id : -1;
}

extern "C" {

struct Tokenizer* q4_tokenizer_new(const char* tokenizer_path, int vocab_size) {   // build_tokenizer :35-59
    FILE* file = fopen(tokenizer_path, "rb");
    if (!file) { fprintf(stderr, "couldn't load %s\n", tokenizer_path); return nullptr; }
    Tokenizer* t = new Tokenizer();
    t->vocab_size = vocab_size;
    t->vocab.resize(vocab_size);
    t->vocab_scores.resize(vocab_size);
    for (int i = 0; i < 256; i++) {
        t->byte_pieces[i * 2] = (unsigned char)i;
        t->byte_pieces[i * 2 + 1] = '\0';
    }
    bool ok = fread(&t->max_token_length, sizeof(int), 1, file) == 1;
    for (int i = 0; ok && i < vocab_size; i++) {
        int len = 0;
        ok = fread(&t->vocab_scores[i], sizeof(float), 1, file) == 1 && fread(&len, sizeof(int), 1, file) == 1 && len >= 0;
        if (!ok) break;
        t->vocab[i].resize(len);
        ok = len == 0 || fread(&t->vocab[i][0], len, 1, file) == 1;
    }
    fclose(file);
    if (!ok) { fprintf(stderr, "failed read\n"); delete t; return nullptr; }
    return t;
}

void q4_tokenizer_delete(struct Tokenizer* t) { delete t; }
int q4_tokenizer_max_token_length(const struct Tokenizer* t) { return (int)t->max_token_length; }
int q4_tokenizer_piece(const struct Tokenizer* t, int id, const char** bytes, int* len) {
    if (!t || !bytes || !len || id < 0 || id >= t->vocab_size) return Q4_ERR_ARG;
    *bytes = t->vocab[id].data();
    *len = (int)t->vocab[id].size();
    return Q4_OK;
}

const char* q4_tokenizer_decode(struct Tokenizer* t, int prev_token, int token) {  // decode :68-79
    const char* piece = t->vocab[token].c_str();
    if (prev_token == bos_token && piece[0] == ' ') piece++;
    unsigned char byte_val;
    if (sscanf(piece, "<0x%02hhX>", &byte_val) == 1) piece = (const char*)t->byte_pieces + byte_val * 2;
    return piece;
}

static void safe_printf(const char* piece) {                                       // tokenizer.h:81-93
    if (piece == NULL || piece[0] == '\0') return;
    if (piece[1] == '\0') {
        unsigned char byte_val = piece[0];
        if (!(isprint(byte_val) || isspace(byte_val))) return;
    }
    printf("%s", piece);
}

int q4_tokenizer_encode(struct Tokenizer* t, const char* text, int bos, int eos, int* tokens, int* n_tokens) {   // encode :102-223
    if (text == NULL) { fprintf(stderr, "cannot encode NULL text\n"); return Q4_ERR_ARG; }
    if (t->sorted_vocab.empty()) {
        t->sorted_vocab.resize(t->vocab_size);
        for (int i = 0; i < t->vocab_size; i++) {
            t->sorted_vocab[i].str = t->vocab[i].c_str();
            t->sorted_vocab[i].id = i;
        }
        qsort(t->sorted_vocab.data(), t->vocab_size, sizeof(TokenIndex), compare_tokens);
    }
    std::vector<char> buf(t->max_token_length * 2 + 1 + 2 + 8);
    char* str_buffer = buf.data();
    size_t str_len = 0;
    *n_tokens = 0;
    if (bos) tokens[(*n_tokens)++] = bos_token;
    if (text[0] != '\0') {                                                         // dummy prefix, :132-136
        int dummy_prefix = str_lookup(" ", t);
        tokens[(*n_tokens)++] = dummy_prefix;
    }
    for (const char* c = text; *c != '\0'; c++) {
        if ((*c & 0xC0) != 0x80) str_len = 0;                                      // not a continuation byte
        str_buffer[str_len++] = *c;
        str_buffer[str_len] = '\0';
        if ((*(c + 1) & 0xC0) == 0x80 && str_len < 4) continue;
        int id = str_lookup(str_buffer, t);
        if (id != -1) {
            tokens[(*n_tokens)++] = id;
        } else {
            for (size_t i = 0; i < str_len; i++) tokens[(*n_tokens)++] = (unsigned char)str_buffer[i] + 3;   // byte fallback
        }
        str_len = 0;
    }
    std::string merged;
    while (1) {                                                                    // greedy best-score merges :186-217
        float best_score = -1e10;
        int best_id = -1, best_idx = -1;
        for (int i = 0; i < (*n_tokens - 1); i++) {
            merged = t->vocab[tokens[i]];
            merged += t->vocab[tokens[i + 1]];
            int id = str_lookup(merged.c_str(), t);
            if (id != -1 && t->vocab_scores[id] > best_score) {
                best_score = t->vocab_scores[id];
                best_id = id;
                best_idx = i;
            }
        }
        if (best_idx == -1) break;
        tokens[best_idx] = best_id;
        for (int i = best_idx + 1; i < (*n_tokens - 1); i++) tokens[i] = tokens[i + 1];
        (*n_tokens)--;
    }
    if (eos) tokens[(*n_tokens)++] = eos_token;
    return Q4_OK;
}

// ---------------------------------------------------------------------------------------------------
static void die_on(int rc) {
    if (rc) { printf("\n%s\n", q4_status_string(rc)); exit(EXIT_FAILURE); }        // the reference's printf + exit
}

// Q4_PROMPT_CACHE=FILE (generate mode): a serialised snapshot of an earlier run's prompt positions. Everything about it goes to stderr; a file that is
// missing, fails q4_snapshot_check or belongs to another model is reported and ignored.
static q4_snapshot* prompt_cache_load(const char* path, Transformer* t) {
    FILE* f = fopen(path, "rb");
    if (!f) return nullptr;                                                        // absent: the run writes it
    std::vector<char> blob;
    long size = -1;
    if (fseek(f, 0, SEEK_END) == 0) size = ftell(f);
    bool ok = size > 0 && fseek(f, 0, SEEK_SET) == 0;
    if (ok) {
        blob.resize((size_t)size);
        ok = fread(blob.data(), 1, blob.size(), f) == blob.size();
    }
    fclose(f);
    q4_snapshot* snap = nullptr;
    if (!ok || q4_snapshot_import(&snap, blob.data(), blob.size()) != Q4_OK) {
        fprintf(stderr, "Q4_PROMPT_CACHE: %s is not a usable snapshot; ignored\n", path);
        return nullptr;
    }
    if (q4_snapshot_restore(t, snap) != Q4_OK) {
        fprintf(stderr, "Q4_PROMPT_CACHE: %s was taken from another model or K / V format; ignored\n", path);
        q4_snapshot_delete(snap);
        return nullptr;
    }
    return snap;
}
static void prompt_cache_save(const char* path, const Transformer* t, int n_pos) {
    q4_snapshot* snap = nullptr;
    struct q4_snapshot_info info;
    if (q4_snapshot_new(&snap, t, n_pos) != Q4_OK) { fprintf(stderr, "Q4_PROMPT_CACHE: no snapshot of %d positions\n", n_pos); return; }
    bool ok = q4_snapshot_info(snap, &info) == Q4_OK;
    std::vector<char> blob;
    if (ok) { blob.resize((size_t)info.export_bytes); ok = q4_snapshot_export(snap, blob.data(), blob.size()) == Q4_OK; }
    q4_snapshot_delete(snap);
    const std::string tmp = std::string(path) + ".tmp";
    FILE* f = ok ? fopen(tmp.c_str(), "wb") : nullptr;
    ok = f && fwrite(blob.data(), 1, blob.size(), f) == blob.size();
    if (f) ok = fclose(f) == 0 && ok;
    if (ok) ok = rename(tmp.c_str(), path) == 0;
    if (!ok) { fprintf(stderr, "Q4_PROMPT_CACHE: cannot write %s\n", path); remove(tmp.c_str()); }
}

// What generate() does with the tokens of the loop: every one is decoded behind its predecessor and printed (llama2_q4.cu:473-476)
struct Printer { struct Tokenizer* tokenizer; const int* prompt_tokens; int vocab_size; };
static void print_token(void* ctx, int, int prev, int next) {
    const Printer* p = (const Printer*)ctx;
    if (next >= p->vocab_size) next = 0;                                               // :474
    safe_printf(q4_tokenizer_decode(p->tokenizer, prev, next));
}
// ... and with an attempt: the second follows a bounded in-launch wait that ran out, the text above is invalid and the library has dropped to fusion
// level 1 (no in-launch waits) -- say so. Each prints what the skipped steps' iterations would, from the prompt's tokens.
static void print_attempt(void* ctx, int attempt, int start) {
    const Printer* p = (const Printer*)ctx;
    if (attempt > 0) printf("\n\n[%s -- generating again]\n", q4_last_error());
    for (int i = 1; i < start; i++) safe_printf(q4_tokenizer_decode(p->tokenizer, p->prompt_tokens[i - 1], p->prompt_tokens[i]));
}

static double generate_cached(Transformer* transformer, struct Tokenizer* tokenizer, Sampler* sampler, const char* prompt, int steps,
                              int* timed_tokens_out, double* seconds_out, const char* cache_path);
// generate(), llama2_q4.cu:436-492
double q4_generate(Transformer* transformer, struct Tokenizer* tokenizer, Sampler* sampler, const char* prompt, int steps,
                   int* timed_tokens_out, double* seconds_out) {
    return generate_cached(transformer, tokenizer, sampler, prompt, steps, timed_tokens_out, seconds_out, nullptr);
}
// ... with a prompt cache (null: none): the positions of the prompt's common prefix with the cached snapshot are not run; their pieces are printed from
// the prompt's tokens, so stdout is what the full run prints
static double generate_cached(Transformer* transformer, struct Tokenizer* tokenizer, Sampler* sampler, const char* prompt, int steps,
                              int* timed_tokens_out, double* seconds_out, const char* cache_path) {
    if (prompt == NULL) prompt = "";
    int num_prompt_tokens = 0;
    int* prompt_tokens = (int*)malloc((strlen(prompt) + 3) * sizeof(int));
    printf("\nEncoding Prompt... ");
    q4_tokenizer_encode(tokenizer, prompt, 1, 0, prompt_tokens, &num_prompt_tokens);
    printf("Done!\n");
    if (num_prompt_tokens < 1) {
        fprintf(stderr, "something is wrong, expected at least 1 prompt token\n");
        exit(EXIT_FAILURE);
    }
    // the prompt cache: restore, then skip the positions the snapshot's tokens share with the prompt -- none of them past an EOS, where the loop stops
    int start_pos = 0, covered = 0;
    if (cache_path) {
        if (q4_snapshot* snap = prompt_cache_load(cache_path, transformer)) {
            struct q4_snapshot_info info;
            die_on(q4_snapshot_info(snap, &info));
            std::vector<int> had(info.n_pos);
            die_on(q4_snapshot_tokens(snap, had.data()));
            while (covered < info.n_pos && covered < num_prompt_tokens && had[covered] == prompt_tokens[covered]) covered++;
            start_pos = covered < num_prompt_tokens - 1 ? covered : num_prompt_tokens - 1;
            if (start_pos > steps) start_pos = 0;
            for (int i = 1; i < start_pos; i++)                                        // (their pieces are printed: no token the loop would clamp)
                if (prompt_tokens[i] >= transformer->config.vocab_size) start_pos = 0;
            die_on(q4_snapshot_delete(snap));                                          // (synchronises: the rows are in place)
        }
    }
    // the token loop (q4_loop.h) over the printer above; q4_set_context_shift: at seq_len the rows slide instead of the loop ending
    Printer printer = {tokenizer, prompt_tokens, transformer->config.vocab_size};
    TokenLoop loop = {print_token, print_attempt, &printer};
    const int rc = q4_token_loop(transformer, sampler, prompt_tokens, num_prompt_tokens, steps, start_pos, &loop);
    printf("\n");
    die_on(rc);
    const int timed_tokens = loop.pos - 1 - loop.start, off = loop.off;                // (the steps this run executed)
    const double time = loop.seconds;
    printf("\nachieved tok/s: %f. Tokens: %d, seconds: %g\n", timed_tokens / time, timed_tokens, time);   // :489
    if (cache_path && off == 0) {      // keep the prompt's positions for the next run, unless the file already covers them
        die_on(q4_stream_synchronize());
        const int done = q4_shared_pos(&transformer->state), n_save = done < num_prompt_tokens ? done : num_prompt_tokens;
        if (n_save >= 1 && covered < n_save) prompt_cache_save(cache_path, transformer, n_save);
    }
    free(prompt_tokens);
    if (timed_tokens_out) *timed_tokens_out = timed_tokens;
    if (seconds_out) *seconds_out = time;
    return timed_tokens / time;
}

static void read_stdin(const char* guide, char* buffer, size_t bufsize) {          // :494-503
    printf("%s", guide);
    if (fgets(buffer, bufsize, stdin) != NULL) {
        size_t len = strlen(buffer);
        if (len > 0 && buffer[len - 1] == '\n') buffer[len - 1] = '\0';
    } else {
        buffer[0] = '\0';
    }
}

// chat(), llama2_q4.cu:507-601
void q4_chat(Transformer* transformer, struct Tokenizer* tokenizer, Sampler* sampler, const char* cli_user_prompt,
             const char* cli_system_prompt, int steps) {
    char system_prompt[512];
    char user_prompt[512];
    char rendered_prompt[1152];
    int num_prompt_tokens = 0;
    int* prompt_tokens = (int*)malloc(1152 * sizeof(int));
    int user_idx = 0;
    int8_t user_turn = 1;
    int next = 0;
    int token = 0;
    int pos = 0;
    RunState* state = &transformer->state;
    // q4_set_context_shift: `pos` counts steps (what `steps` bounds); the ring index and the step's position are the device's, which a shift lowers
    int shift_keep = 0, shift_discard = 0;
    (void)q4_get_context_shift(transformer, &shift_keep, &shift_discard);
    system_prompt[0] = '\0';
    die_on(q4_reset_sequence(state, nullptr, 0));                                  // :526-527
    while (pos < steps) {
        if (user_turn) {
            if (feof(stdin)) break;   // scripted stdin ran dry (the reference would spin on empty prompts)
            if (pos == 0) {
                if (cli_system_prompt == NULL) read_stdin("Enter system prompt (optional): ", system_prompt, sizeof(system_prompt));
                else { strncpy(system_prompt, cli_system_prompt, sizeof(system_prompt) - 1); system_prompt[sizeof(system_prompt) - 1] = 0; }
            }
            if (pos == 0 && cli_user_prompt != NULL) { strncpy(user_prompt, cli_user_prompt, sizeof(user_prompt) - 1); user_prompt[sizeof(user_prompt) - 1] = 0; }
            else read_stdin("User: ", user_prompt, sizeof(user_prompt));
            if (pos == 0 && system_prompt[0] != '\0')
                snprintf(rendered_prompt, sizeof(rendered_prompt), "[INST] <<SYS>>\n%s\n<</SYS>>\n\n%s [/INST]", system_prompt, user_prompt);
            else
                snprintf(rendered_prompt, sizeof(rendered_prompt), "[INST] %s [/INST]", user_prompt);
            printf("\nRendered prompt: %s\n", rendered_prompt);                    // :564
            q4_tokenizer_encode(tokenizer, rendered_prompt, 1, 0, prompt_tokens, &num_prompt_tokens);
            user_idx = 0;
            user_turn = 0;
            printf("Assistant: ");
            die_on(q4_stream_synchronize());
            const int at = q4_shared_pos(state);
            for (int i = 0; i < num_prompt_tokens && at + i < Q4_MAX_SEQ_LEN; i++)
                transformer->state.shared_data->tokens[at + i] = prompt_tokens[i];    // :573
        }
        die_on(q4_stream_synchronize());                                           // :578
        if (shift_discard > 0 && q4_shared_pos(state) == transformer->config.seq_len) {   // the ring behind the position: the token the last step chose, or the turn's tokens that still wait
            const int waiting = num_prompt_tokens - user_idx > 1 ? num_prompt_tokens - user_idx : 1;
            const int n_ring = transformer->config.seq_len + waiting < Q4_MAX_SEQ_LEN ? transformer->config.seq_len + waiting : Q4_MAX_SEQ_LEN;
            die_on(q4_shift_context(transformer, transformer->config.seq_len, shift_keep, shift_discard, n_ring));
        }
        const int at = q4_shared_pos(state);
        // (q4_run_transformer's step; a greedy generating step may screen its classifier: only its token is read. Not the last one.)
        die_on(run_transformer_steps_screenable(at, 1, user_idx >= num_prompt_tokens - 1, &transformer->config, state, &transformer->weights, 0, sampler, group_may_screen(pos, 1, steps)));
        user_idx++;
        if (user_idx > 0) {
            next = q4_shared_token(state, at);                                     // :584
            if (next == eos_token) {
                user_turn = 1;
                printf("\n");
                if (q4_handoff_status(state)) {   // the turn just printed came out of a timed-out in-launch wait: say so, stop
                    printf("\n%s\n", q4_last_error());
                    break;
                }
            } else if (user_idx > num_prompt_tokens) {
                const char* piece = q4_tokenizer_decode(tokenizer, token, next);
                safe_printf(piece);
            }
            token = next;
        }
        pos++;
    }
    printf("\n");
    if (q4_handoff_status(state)) printf("\n%s\n", q4_last_error());
    free(prompt_tokens);
}

// get_dataset_perplexity, perplexity.h:57-97
float q4_get_dataset_perplexity(char* dataset, struct Tokenizer* tokenizer, Transformer* t, Sampler* sampler) {
    int bytes = strlen(dataset);
    Config* config = &t->config;
    std::vector<int> toks(bytes + 4);
    printf("\nTokenizing Dataset...");
    int totalTokens = 0;
    toks[0] = bos_token;                                                           // :78
    q4_tokenizer_encode(tokenizer, dataset, 0, 0, toks.data() + 1, &totalTokens);  // :63
    printf("done!\n");
    printf("Found %d characters, %d tokens", bytes, totalTokens);
    int numTokens = totalTokens;
    if (numTokens >= config->seq_len) {
        numTokens = config->seq_len - 1;
        printf("\nTruncated to %d tokens", numTokens);
    }
    printf("\nRunning the network to get logits...");
    float pplx = q4_perplexity_ids(t, sampler, toks.data(), numTokens);            // :74-91
    printf("done!\n");
    printf("Computing perplexity...");
    printf("\nPerplexity computed on %d tokens: %f\n\n", numTokens, pplx);         // :93
    return pplx;
}

// parseDataSetAndComputePreplexity, perplexity.h:99-139
double q4_parse_dataset_and_compute_perplexity(const char* textFileName, struct Tokenizer* tokenizer, Transformer* t,
                                               Sampler* sampler) {
    FILE* fp = fopen(textFileName, "rb");
    if (!fp) { printf("Couldn't open file %s\n", textFileName ? textFileName : "(null)"); return -1.0; }
    printf("\nLoading Dataset...");
    fseek(fp, 0, SEEK_END);
    long bytes = ftell(fp);
    fseek(fp, 0, SEEK_SET);
    char* dataset = (char*)malloc(bytes + 1);
    if (fread(dataset, 1, bytes, fp) != (size_t)bytes) bytes = 0;
    fclose(fp);
    printf("done!\n");
    dataset[bytes] = 0;
    int count = 0;
    double pplx_product = 1;
    char* currentSeq = dataset;
    while (currentSeq) {
        char* nextseq = strstr(currentSeq, "<|endoftext|>");
        if (nextseq) {
            *nextseq = 0;
            nextseq += 13;
            pplx_product *= q4_get_dataset_perplexity(currentSeq, tokenizer, t, sampler);
            count++;
            currentSeq = nextseq;
        } else {
            pplx_product *= q4_get_dataset_perplexity(currentSeq, tokenizer, t, sampler);
            count++;
            break;
        }
    }
    free(dataset);
    double geo = pow(pplx_product, 1.0 / count);
    printf("\nGeomean perplexity on %d sequences: %f\n\n", count, geo);            // :138
    return geo;
}

// ---------------------------------------------------------------------------------------------------
// CLI, llama2_q4.cu:604-720
static void error_usage_text(const char* argv0) {
    fprintf(stderr, "Usage:   %s <checkpoint> [options]\n", argv0);
    fprintf(stderr, "Example: %s model.bin -n 256 -i \"Write a poem on GPUs\"\n", argv0);
    fprintf(stderr, "Options:\n");
    fprintf(stderr, "  -n <int>    max number of steps to run for, default = max_seq_len\n");
    fprintf(stderr, "  -i <string> input prompt\n");
    fprintf(stderr, "  -f <string> path to file containing input prompt. Can be used with for multi-line prompts.\n");
    fprintf(stderr, "  -t <float>  temperature in [0,inf], default 0.5\n");
    fprintf(stderr, "  -p <float>  p value in top-p (nucleus) sampling in [0,1] default 0.9\n");
    fprintf(stderr, "  -s <int>    random seed, default time(NULL)\n");
    fprintf(stderr, "  -z <string> optional path to custom tokenizer\n");
    fprintf(stderr, "  -m <string> mode: generate|chat|perplexity, default: generate\n");
    fprintf(stderr, "  -y <string> (optional) system prompt in chat mode\n");
    fprintf(stderr, "  -q <string> dataset file for computing perplexity\n");
}

static std::string g_file_prompt;

int q4_parse_args(int argc, char** argv, q4_cli_args* a) {
    // defaults, llama2_q4.cu:624-637
    a->checkpoint_path = NULL;
    a->tokenizer_path = "tokenizer.bin";
    a->dataset_path = NULL;
    a->steps = 0;
    a->prompt = NULL;
    a->perplexity = 0;
    a->temperature = 0.5f;
    a->topp = 0.6f;          // the code default (help text says 0.9)
    a->rng_seed = 0;
    a->mode = "generate";
    a->system_prompt = NULL;
    a->seed_from_time = 0;
    if (argc >= 2) a->checkpoint_path = argv[1]; else return 1;
    for (int i = 2; i < argc; i += 2) {
        if (i + 1 >= argc) return 1;
        if (argv[i][0] != '-') return 1;
        if (strlen(argv[i]) != 2) return 1;
        switch (argv[i][1]) {
            case 'n': a->steps = atoi(argv[i + 1]); break;
            case 'i': a->prompt = argv[i + 1]; break;
            case 'z': a->tokenizer_path = argv[i + 1]; break;
            case 't': a->temperature = atof(argv[i + 1]); break;
            case 'p': a->topp = atof(argv[i + 1]); break;
            case 's': a->rng_seed = atoi(argv[i + 1]); break;                     // atoi into 64 bits, P9
            case 'm': a->mode = argv[i + 1]; break;
            case 'y': a->system_prompt = argv[i + 1]; break;
            case 'q': a->dataset_path = argv[i + 1]; break;
            case 'f': {
                FILE* file = fopen(argv[i + 1], "r");
                if (!file) { printf("Couldn't open file %s\n", argv[i + 1]); exit(1); }
                fseek(file, 0, SEEK_END);
                long fsize = ftell(file);
                fseek(file, 0, SEEK_SET);
                if (a->prompt) printf("Warning: -f overrides -i\n");
                g_file_prompt.resize(fsize);
                if (fsize > 0 && fread(&g_file_prompt[0], fsize, 1, file) != 1) g_file_prompt.clear();
                fclose(file);
                a->prompt = g_file_prompt.c_str();
                break;
            }
            default: return 1;
        }
    }
    if (strcmp(a->mode, "perplexity") == 0) a->perplexity = 1;                     // :678
    // parameter validation/overrides :681-685
    if (a->rng_seed <= 0) { a->rng_seed = (unsigned int)time(NULL); a->seed_from_time = 1; }
    if (a->temperature < 0.0) a->temperature = 0.0;
    if (a->topp < 0.0 || 1.0 < a->topp) a->topp = 0.9;
    return 0;
}

// Q4_DRY_BREAKERS: "default" -- every token whose piece holds a newline, ':', '"' or '*' (a byte-fallback piece <0xHH> counts as its byte) -- or a list
// of ids; false: not a list of numbers below the vocabulary
static bool dry_breakers_from(const char* text, const struct Tokenizer* tokenizer, int vocab, std::vector<int>* ids) {
    if (strcmp(text, "default") == 0) {
        for (int id = 0; id < vocab; id++) {
            const char* piece = nullptr;
            int len = 0;
            if (q4_tokenizer_piece(tokenizer, id, &piece, &len) || len <= 0) continue;
            char byte = 0;
            if (len == 6 && !memcmp(piece, "<0x", 3) && piece[5] == '>' && isxdigit((unsigned char)piece[3]) && isxdigit((unsigned char)piece[4])) {
                const char hex[3] = {piece[3], piece[4], 0};
                byte = (char)strtol(hex, nullptr, 16);
                piece = &byte;
                len = 1;
            }
            for (int i = 0; i < len; i++)
                if (piece[i] == '\n' || piece[i] == ':' || piece[i] == '"' || piece[i] == '*') { ids->push_back(id); break; }
        }
        return true;
    }
    for (const char* p = text; *p;) {
        if (*p < '0' || *p > '9') return false;
        char* rest = nullptr;
        const long v = strtol(p, &rest, 10);
        if (v >= vocab || (*rest && *rest != ',') || (*rest == ',' && !rest[1])) return false;
        ids->push_back((int)v);
        p = *rest ? rest + 1 : rest;
    }
    return true;
}

int q4_main(int argc, char** argv) {
    q4_cli_args a;
    if (q4_parse_args(argc, argv, &a)) { error_usage_text(argv[0]); exit(EXIT_FAILURE); }
    if (!a.perplexity && a.dataset_path) printf("Warning: dataset path is ignored in non-perplexity mode\n");

    // the K / V cache format comes from the environment: the flags, CliArgs and the usage text stay the reference's
    const char* kv = getenv("Q4_KV_CACHE");
    if (kv && strcmp(kv, "fp8") == 0) q4_set_kv_format(Q4_KV_FP8);
    else if (kv && *kv && strcmp(kv, "fp16") != 0) { fprintf(stderr, "Q4_KV_CACHE: unknown format '%s' (fp16 or fp8)\n", kv); exit(EXIT_FAILURE); }
    // ... the RoPE scaling of the model (q4_parse_rope_scaling): Q4_ROPE_SCALING="llama3,factor=8,low=1,high=4,orig=8192"
    const char* rope = getenv("Q4_ROPE_SCALING");
    q4_rope_scaling scaling;
    if (rope && *rope && (q4_parse_rope_scaling(rope, &scaling) || q4_set_rope_scaling(&scaling))) {
        fprintf(stderr, "Q4_ROPE_SCALING: cannot use '%s' (none | linear,factor=F | llama3,factor=F,low=L,high=H,orig=N; F >= 1, 0 < L < H, N >= 1; "
                        "e.g. llama3,factor=8,low=1,high=4,orig=8192)\n", rope);
        exit(EXIT_FAILURE);
    }
    // ... and so do the sampling controls (q4_parse_sampling_controls): Q4_SAMPLING="top_k=40,min_p=0.05,repeat_penalty=1.1,last_n=64"
    const char* sampling = getenv("Q4_SAMPLING");
    q4_sampling_controls controls;
    if (sampling && *sampling && q4_parse_sampling_controls(sampling, &controls)) {
        fprintf(stderr, "Q4_SAMPLING: cannot use '%s' (keys: top_k, min_p, repeat_penalty, last_n, presence, frequency; e.g. top_k=40,repeat_penalty=1.1)\n", sampling);
        exit(EXIT_FAILURE);
    }
    // ... and DRY / the n-gram ban (q4_parse_dry): Q4_DRY="multiplier=0.8,ngram=4"; Q4_DRY_BREAKERS: a comma-separated id list, or "default"
    const char* dry_text = getenv("Q4_DRY");
    q4_dry_controls dry;
    if (dry_text && *dry_text && q4_parse_dry(dry_text, &dry)) {
        fprintf(stderr, "Q4_DRY: cannot use '%s' (keys: multiplier, base, allowed, last_n, ngram; e.g. multiplier=0.8,base=1.75,allowed=2,last_n=1024)\n", dry_text);
        exit(EXIT_FAILURE);
    }
    // ... and typical-p / top-n-sigma / Mirostat v2 (q4_parse_adaptive): Q4_ADAPTIVE="typical_p=0.9" or "mirostat_tau=5,mirostat_eta=0.1"
    const char* adaptive_text = getenv("Q4_ADAPTIVE");
    q4_adaptive_controls adaptive;
    if (adaptive_text && *adaptive_text && q4_parse_adaptive(adaptive_text, &adaptive)) {
        fprintf(stderr, "Q4_ADAPTIVE: cannot use '%s' (keys: typical_p, top_n_sigma, mirostat_tau, mirostat_eta; e.g. typical_p=0.9 or mirostat_tau=5,mirostat_eta=0.1)\n", adaptive_text);
        exit(EXIT_FAILURE);
    }

    Transformer transformer;
    int rc = q4_build_transformer(&transformer, a.checkpoint_path, a.perplexity);
    if (rc) exit(rc == Q4_ERR_IO ? 1 : EXIT_FAILURE);
    // ... and the context shift (q4_parse_context_shift): Q4_CONTEXT_SHIFT="keep=4,discard=256"; with it -n may pass seq_len
    const char* shift = getenv("Q4_CONTEXT_SHIFT");
    const bool shifting = shift && *shift;
    if (shifting) {
        int keep = 0, discard = 0;
        if (q4_parse_context_shift(shift, &keep, &discard) || q4_set_context_shift(&transformer, keep, discard)) {
            fprintf(stderr, "Q4_CONTEXT_SHIFT: cannot use '%s' (keys: keep, discard; discard >= 1, keep + discard <= %d; e.g. keep=4,discard=256)\n", shift, transformer.config.seq_len);
            exit(EXIT_FAILURE);
        }
    }
    // ... and speculative greedy decoding (q4_parse_speculative): Q4_SPECULATIVE="draft=4,ngram=3,min=2"; runs that are not greedy keep their steps unless Q4_SPECULATIVE_SAMPLED says otherwise
    const char* spec = getenv("Q4_SPECULATIVE");
    if (spec && *spec) {
        int draft = 0, ngram = 0, ngram_min = 0;
        if (q4_parse_speculative(spec, &draft, &ngram, &ngram_min) || q4_set_speculative(&transformer, draft, ngram, ngram_min)) {
            fprintf(stderr, "Q4_SPECULATIVE: cannot use '%s' (keys: draft, ngram, min; draft 0 .. %d, 1 <= min <= ngram <= %d; e.g. draft=4,ngram=3,min=2)\n", spec, Q4_SPEC_MAX_DRAFT, Q4_SPEC_MAX_NGRAM);
            exit(EXIT_FAILURE);
        }
    }
    // ... and verify passes under the temperature / top-p sampler (q4_set_speculative_sampled), a variable of its own: Q4_SPECULATIVE_SAMPLED=1
    const char* spec_sampled = getenv("Q4_SPECULATIVE_SAMPLED");
    if (spec_sampled && *spec_sampled) {
        int on = 0;
        if (q4_parse_speculative_sampled(spec_sampled, &on) || q4_set_speculative_sampled(&transformer, on)) {
            fprintf(stderr, "Q4_SPECULATIVE_SAMPLED: cannot use '%s' (0 or 1: verify passes also under the temperature / top-p sampler; needs Q4_SPECULATIVE)\n", spec_sampled);
            exit(EXIT_FAILURE);
        }
    }
    // ... and passes for the grouped-query 4096-wide shape (q4_set_pass_gqa): Q4_PASS_GQA=1
    const char* pass_gqa = getenv("Q4_PASS_GQA");
    if (pass_gqa && *pass_gqa) {
        int on = 0;
        if (q4_parse_pass_gqa(pass_gqa, &on) || q4_set_pass_gqa(&transformer, on)) {
            fprintf(stderr, "Q4_PASS_GQA: cannot use '%s' (0 or 1: prompt and verify passes also for grouped-query models of dim 4096, e.g. Mistral-7B, Llama-3-8B)\n", pass_gqa);
            exit(EXIT_FAILURE);
        }
    }
    // ... and passes for a model with the FP8 K / V cache (q4_set_pass_kv8): Q4_PASS_KV8=1
    const char* pass_kv8 = getenv("Q4_PASS_KV8");
    if (pass_kv8 && *pass_kv8) {
        int on = 0;
        if (q4_parse_pass_kv8(pass_kv8, &on) || q4_set_pass_kv8(&transformer, on)) {
            fprintf(stderr, "Q4_PASS_KV8: cannot use '%s' (0 or 1: prompt and verify passes also with Q4_KV_CACHE=fp8)\n", pass_kv8);
            exit(EXIT_FAILURE);
        }
    }
    // ... and passes for Llama-2-13B's shape (q4_set_pass_13b): Q4_PASS_13B=1
    const char* pass_13b = getenv("Q4_PASS_13B");
    if (pass_13b && *pass_13b) {
        int on = 0;
        if (q4_parse_pass_13b(pass_13b, &on) || q4_set_pass_13b(&transformer, on)) {
            fprintf(stderr, "Q4_PASS_13B: cannot use '%s' (0 or 1: prompt and verify passes also for models of dim 5120 and hidden 13824, e.g. Llama-2-13B)\n", pass_13b);
            exit(EXIT_FAILURE);
        }
    }
    // ... and passes while logit stages are on, with the guide's forced drafts (q4_set_pass_stages): Q4_PASS_STAGES=1
    const char* pass_stages = getenv("Q4_PASS_STAGES");
    if (pass_stages && *pass_stages) {
        int on = 0;
        if (q4_parse_pass_stages(pass_stages, &on) || q4_set_pass_stages(&transformer, on)) {
            fprintf(stderr, "Q4_PASS_STAGES: cannot use '%s' (0 or 1: verify passes also with a guide, DRY or the sampling controls on, prompt passes also with a guide or Mirostat)\n", pass_stages);
            exit(EXIT_FAILURE);
        }
    }
    // ... and how far prompt and verify passes go (q4_set_pass_context): Q4_PASS_CONTEXT=2048; values up to 256 are the default
    const char* pass_context = getenv("Q4_PASS_CONTEXT");
    if (pass_context && *pass_context) {
        char* rest = nullptr;
        const long v = pass_context[0] >= '0' && pass_context[0] <= '9' ? strtol(pass_context, &rest, 10) : -1;     // (no sign, no leading blank)
        if (v < 0 || !rest || *rest || v > Q4_MAX_SEQ_LEN) {
            fprintf(stderr, "Q4_PASS_CONTEXT: cannot use '%s' (one integer, 0 .. %d: the positions below which prompt and verify passes run; e.g. 2048)\n", pass_context, Q4_MAX_SEQ_LEN);
            exit(EXIT_FAILURE);
        }
        q4_set_pass_context((int)v);
    }
    int steps = a.steps;
    if (steps <= 0 || (!shifting && steps > transformer.config.seq_len)) steps = transformer.config.seq_len;   // :690
    if (shifting && steps > Q4_MAX_SEQ_LEN - 1) steps = Q4_MAX_SEQ_LEN - 1;

    struct Tokenizer* tokenizer = q4_tokenizer_new(a.tokenizer_path, transformer.config.vocab_size);
    if (!tokenizer) exit(EXIT_FAILURE);
    Sampler sampler;
    die_on(build_sampler(&sampler, transformer.config.vocab_size, a.temperature, a.topp, a.rng_seed));
    if (sampling && *sampling) die_on(q4_sampler_set_controls(&sampler, &controls));
    if (dry_text && *dry_text) die_on(q4_sampler_set_dry(&sampler, &dry));
    if (adaptive_text && *adaptive_text) die_on(q4_sampler_set_adaptive(&sampler, &adaptive));
    const char* breakers = getenv("Q4_DRY_BREAKERS");
    if (breakers && *breakers) {
        std::vector<int> ids;
        if (!dry_breakers_from(breakers, tokenizer, transformer.config.vocab_size, &ids) || q4_sampler_set_dry_breakers(&sampler, ids.data(), (int)ids.size())) {
            fprintf(stderr, "Q4_DRY_BREAKERS: cannot use '%s' (distinct token ids below %d, e.g. 13,29901 -- or default: every token with a newline, ':', '\"' or '*' in it)\n",
                    breakers, transformer.config.vocab_size);
            exit(EXIT_FAILURE);
        }
    }

    q4_stream_t stream;
    die_on(q4_stream_create(&stream));                                             // :700
    q4_set_stream(stream);

    if (a.perplexity) {
        q4_parse_dataset_and_compute_perplexity(a.dataset_path, tokenizer, &transformer, &sampler);
    } else if (strcmp(a.mode, "generate") == 0) {
        // Q4_PROMPT_CACHE=FILE: the prompt's K / V rows are kept in FILE and reused by the next run that shares a prefix with it
        const char* cache = getenv("Q4_PROMPT_CACHE");
        generate_cached(&transformer, tokenizer, &sampler, a.prompt, steps, nullptr, nullptr, cache && *cache ? cache : nullptr);
    } else if (strcmp(a.mode, "chat") == 0) {
        q4_chat(&transformer, tokenizer, &sampler, a.prompt, a.system_prompt, steps);
    } else {
        error_usage_text(argv[0]);
        exit(EXIT_FAILURE);
    }
    q4_stream_synchronize();
    q4_reset_graphs();                                                             // :713-716
    q4_free_transformer(&transformer);
    destroy_sampler(&sampler);
    q4_set_stream(nullptr);
    q4_stream_destroy(stream);
    q4_tokenizer_delete(tokenizer);
    return 0;
}

}  // extern "C"
