// The mark of a checker's exported functions: tests/native_libs.py builds every file here with -fvisibility=hidden and reads each function's ctypes signature
// from the `HOST_API <ret> name(<args>)` line that defines it.
#define HOST_API extern "C" __attribute__((visibility("default")))
